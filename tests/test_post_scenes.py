"""The post chain -- the guide kernels k_denoise_guides / k_denoise_guides_cov with the a-trous passes behind them (brt_denoise.hip),
k_temporal (brt_temporal.hip), k_upscale in its three packs (plain, UpscaleBlend, UpscaleSelect; brt_upscale.hip) and k_adaptive_select
with the pixel re-trace behind it (brt_adaptive.hip) -- on general trees and hostile scenes: the 40 randomized and 40 wild scenes of
tests/shade_cases.py, each under its own tree and under a median-split tree of three-sphere leaves, and the lane boards under one leaf
of every sphere.  (tests/test_denoise*.py, test_temporal*.py, test_blend_post.py, test_upscale*.py and test_adaptive*.py upload generated
scenes and hand-made ones of one or two spheres: sane materials under simple trees.)

Every input of a GPU call comes from the C oracle and is uploaded: the noisy frame of brt_denoise_device, the low frame of the upscale
calls, the base frame of the adaptive and refine calls, the coverage frame of brt_blend_post_device -- Pure level, the scene's own
window, the sample count clipped to 1..5 for the filters (both sides of the strength switch at 4) and to 1..3 for upscale and adaptive.
Every expectation is a restatement (denoise_ref, temporal_ref, blend_post_ref, upscale_ref, upscale_blend_ref, upscale_refine_ref,
adaptive_ref, and the float64 denoise_ref64 / upscale_ref64) fed with denoise_ref.guides of the oracle on the twin of the tree the GPU
walked; brt_debug_denoise_guides is itself under test (item 1) and feeds nothing.

  * CPU: the tables are what they claim, on the oracle alone (the counts printed, the floors a little below them): views that hit and
    miss, no NaN in a guide plane, guides that differ between a wild scene's own tree and the median split, non-finite oracle colours,
    scenes with filtered pixels, the three upscale stages, both classes of both masks, coverage frames with both classes, no tie in
    temporal_ref.sphere_ids; the f32 restatements stay inside the 1e-4 bar against the float64 ones, pass-through pixels are bit-equal.
  * GPU: (1) all eight guide planes as bits; (2) brt_denoise_device at 1, 3 and 5 iterations and one other sigma set, three packed
    formats; (3) brt_blend_post_device on the level-1/2 scenes; (4) brt_upscale_device, brt_upscale_blend_device,
    brt_upscale_refine_mask_device and brt_upscale_refine_device (the re-trace under three residencies and in the plain form, rotating);
    (5) brt_adaptive_mask_device and brt_adaptive_refine_device; (6) three-frame temporal sequences on the randomized table.

What is bitwise (a NaN equals a NaN at the same place: test_gbuffer._canon): the guides, pass-through and covered pixels, sky pixels
of the upscaler, both class masks and their counts, every re-traced pixel, the adaptive frame, the packed formats as the store of the
f32 result.  What is held to |got - want| <= 1e-4 max(1, |want|) (DESIGN.md sections 10 and 14; where `want` is not finite: the same
class): filtered pixels, stages A, B, C, temporal frames; the temporal state by test_temporal._compare_state with no pixel excused.

A window of height 0 (wild scenes 0 and 25): camera_ray_dir_center adds (1 / window size) * 0 to the pixel's position, INF * 0 there,
so every guide ray is NaN and misses, as every ray of the frame does.  denoise_ref.pixel_center_rays restates the term (`window`); the
low frame's window is max(1, .), so those two views upsample a low frame with hits to an all-sky output of NaN sky colours.

The hot order cannot renumber a general tree: prepass_order counts record visits only for 16-bit descriptors, a simple tree and more
than 64 pair records walked from the LDS tile (brt_api_order.cpp), so rmap stays null under median3.  The scenes of the tables are
too small to tell which condition binds (at most 58 spheres in the randomized table): test_no_hot_order_on_a_general_tree takes the
10 004-sphere grid, which meets every condition but the tree's, asserts that its pre-pass ran with the top of the tree in LDS and
hot_records == 0 under median3, and hot_records > 64 for the same spheres under the callee's simple tree.  (Measured: 0 on all three
frames of the general tree, 4 486 records renumbered by the control's first frame.)

Measured where this file was written (one MI355X; DESIGN.md section 17, "The post chain on hard scenes"; the tests print the figures).
The table counts on the oracle, randomized / wild: scenes with a hit 39 / 29, with hit and miss 34 / 14 (31 / 15 without the window
term: wild scenes 0 and 25 have a window of height 0 and see nothing), a NaN in a guide plane 0 / 0, guides that differ between the own
tree and median3 0 / 9, frames with non-finite colours 0 / 9, scenes with a filtered pixel 39 / 29, stage pixels A 24 526 / 50 469,
B 69 / 66, C 192 / 77, sky 17 965 / 40 035, none 0 / 14, scenes with stage B 23 / 10 and stage C 26 / 16, adaptive masks that select
some and not all 38 / 23, refine masks 36 / 16, sphere_ids ties 0 of 24 787 / 0 of 50 626 hit pixels, level-1/2 scenes 23 (8 with
their own raster inputs) / 17 (5), coverage frames with both classes 22 / 12; f32 against float64: denoise at 3 iterations 1.78e-5 /
5.43e-5, upscale 2.03e-6 / 2.64e-6, stages equal everywhere.
The worst GPU error against the f32 restatement, randomized / wild: denoise 1.28e-5 / 8.79e-5, blend-post 6.14e-6 / 5.96e-7, upscale
2.38e-7 / 2.38e-7 (against float64 2.03e-6 / 2.64e-6), upscale-blend 2.38e-7 / 1.79e-7, temporal frames 2.43e-5 (randomized only); the
guides, both masks, the counts, the refined and the adaptive frames bitwise.  No entry point refused any view (0 refusals in every
family and table).  169 spheres move in the temporal sequences and 24 263 pixels keep a history through the third frame under either
tree.  Wall time: the 17 CPU tests 10.4 s, the 29 GPU tests 11.5 s with their share of the oracle; the slowest GPU case 1.1 s (the
temporal sequences under median3: 120 oracle frames and 40 more guide frames), no other above 0.7 s.

Two deliberate one-line breaks, each tried on a scratch copy of the library -- `plain = !(m1.w > 0.0f)` for `plain = m1.w == 0.0f`, which
takes a negative or NaN specular_transmission for "not refracting".  In denoise_guides_pixel: tests/test_denoise.py,
test_denoise_edges.py, test_blend_post.py and test_temporal.py stay green (71 passed); 8 tests fail here (the guides of the wild table
under both trees and of the boards under both trees, denoise and upscale on the wild table under both trees).  In k_upscale's own copy
alone: tests/test_upscale.py, test_upscale_synthetic.py, test_upscale_blend.py and test_upscale_refine.py stay green (182 passed); 2
tests fail here (upscale on the wild table under both trees: the remodulation a of the output pixel no longer moves with the low
guides')."""
import functools

import numpy as np
import pytest

import bevyray_amd as brt
import adaptive_ref as ar
import blend_post_ref as bp
import denoise_ref as dr
import denoise_ref64 as dr64
import shade_cases as sc
import temporal_ref as tr
import upscale_blend_ref as ubr
import upscale_ref as ur
import upscale_ref64 as ur64
import upscale_refine_ref as rr
from test_gbuffer import _canon
from test_list_tracers_scenes import LENS_BOARDS, RESIDENCIES, TREES, _board, _pure, flavour
from test_temporal import _compare_state, _rel

F32 = np.float32
U32 = np.uint32
BAR = 1e-4                                                   # DESIGN.md sections 10 and 14, tests/test_denoise.py
SCENE_TREES = ("ploc", "median3")                            # "ploc": the scene's own tree, as test_list_tracers_scenes names it
MAX_REFUSED = 4                                              # views of a table an entry point may refuse by a documented rule
_SCENES = {"random": sc.random_scenes, "wild": sc.wild_scenes}
KINDS = list(_SCENES)
ITERATIONS = (1, 3, 5)
OTHER_SIGMAS = dict(iterations=3, sigma_l=2.5, sigma_n=32.0, sigma_z=0.5)
PACKED = ((brt.FLAG_OUT_RGBA8_UNORM_SRGB, "srgb8"), (brt.FLAG_OUT_RGBA8_UNORM, "unorm8"), (brt.FLAG_OUT_RGBA16F, "f16"))
BOTH = brt.REFINE_EDGES | brt.REFINE_SPECULAR
ADAPT_MORE = 2                                               # the adaptive re-trace runs at the base frame's samples + 2
RETRACE_RUNS = ("lds", "lds_top", "global", "plain")
# the floors of the case tables, a little below what the oracle gave here (the tests print the counts)
MIN_WITH_A_HIT = {"random": 36, "wild": 27}                  # 39, 29
MIN_HIT_AND_MISS = {"random": 30, "wild": 12}                # 34, 14
MIN_TREES_DIFFER = {"random": 0, "wild": 7}                  # 0 (asserted as 0), 9
MIN_NON_FINITE = {"random": 0, "wild": 7}                    # 0 (asserted as 0), 9
MIN_FILTERED = {"random": 36, "wild": 26}                    # scenes with a filtered pixel: 39, 29
MIN_STAGE_B = {"random": 20, "wild": 9}                      # 23, 10
MIN_STAGE_C = {"random": 23, "wild": 14}                     # 26, 16
# output pixels per upscale stage over a table: A 24 526 / 50 469, B 69 / 66, C 192 / 77, sky 17 965 / 40 035
MIN_STAGE_PIXELS = {"random": {"A": 23000, "B": 60, "C": 170, "SKY": 17000}, "wild": {"A": 48000, "B": 58, "C": 68, "SKY": 38000}}
MIN_ADAPTIVE_MIXED = {"random": 35, "wild": 20}              # 38, 23
MIN_REFINE_MIXED = {"random": 33, "wild": 14}                # 36, 16
MIN_BLENDED = {"random": 23, "wild": 17}                     # level-1/2 scenes: exactly these
OWN_RASTER = {"random": 8, "wild": 5}                        # ... of which with their own raster inputs: exactly these
MIN_COVERAGE_MIXED = {"random": 19, "wild": 10}              # 22, 12


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _canon_same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(_canon(a), _canon(b))


def _held(got, want):
    """The largest |got - want| / max(1, |want|) where `want` is finite; where it is not, `got` must be of the same class (NaN, +INF,
    -INF) -- upscale_ref64.compare's reading of the bar."""
    err, same = ur64.compare(got, want)
    assert same, "a value that is not finite in the reference differs in class"
    return err


# ---- the scenes and what the oracle says of them, once ---------------------------------------------------------------------------------

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


@functools.lru_cache(maxsize=None)
def _scene(kind, i, tree):
    b, lvl, cam, win, w, h = _SCENES[kind]()[i][:6]
    return TREES[tree](b), lvl, cam, win, w, h


def _at(cam, n):
    c = cam.copy()
    c["sample_count"] = n
    return c


def _spp(cam, hi):
    return int(np.clip(int(cam[0]["sample_count"]), 1, hi))


def _low(kind, i):
    """(low width, low height, the low frame's window)"""
    _, _, _, win, w, h = _scene(kind, i, "ploc")
    lw, lh = (w + 1) // 2, (h + 1) // 2
    return lw, lh, brt.upscale_window(win, h, lh)


def _size_window(kind, i, low):
    _, _, _, win, w, h = _scene(kind, i, "ploc")
    return _low(kind, i) if low else (w, h, win)


def _guides(oracle, kind, i, tree, low=False):
    w, h, win = _size_window(kind, i, low)
    b, _, cam = _scene(kind, i, tree)[:3]
    return _once(("guides", kind, i, tree, low), lambda: dr.guides(oracle, b, cam, w, h, window=win))


def _rays(oracle, kind, i, low=False):
    """(directions (h, w, 3), tan(fov / 2)) of the pixel-centre rays as the kernels cast them"""
    w, h, win = _size_window(kind, i, low)
    cam = _scene(kind, i, "ploc")[2]
    return _once(("rays", kind, i, low), lambda: dr.pixel_center_rays(oracle, cam, w, h, window=win)[1:])


def _frame(oracle, kind, i, tree, n, low=False):
    """The oracle's Pure frame of the scene under `tree` at n samples, at full size or at the low size with the low window."""
    w, h, win = _size_window(kind, i, low)
    b, lvl, cam = _scene(kind, i, tree)[:3]
    return _once(("frame", kind, i, tree, n, low), lambda: np.asarray(oracle.render(b, _pure(lvl), _at(cam, n), win, w, h)[0], F32))


def _blended(kind, i):
    """None for a scene of level 0 or 3, else (raster colour, raster depth): its own, or blend_post_ref's fixture."""
    case = _SCENES[kind]()[i]
    if int(case[1]["level"][0]) not in (1, 2):
        return None
    w, h = case[4], case[5]
    if case[6] is not None:
        return np.asarray(case[6], F32), np.asarray(case[7], F32)
    return bp.raster_inputs(w, h)


def _coverage_frame(oracle, kind, i, tree):
    """The level's frame traced with the raster depth and no raster colour, at the filters' sample count."""
    b, lvl, cam, win, w, h = _scene(kind, i, tree)
    depth = _blended(kind, i)[1]
    return _once(("coverage", kind, i, tree), lambda: np.asarray(oracle.render(b, lvl, _at(cam, _spp(cam, 5)), win, w, h, None, depth)[0], F32))


def _denoise_want(oracle, kind, i, tree, settings):
    frame = _frame(oracle, kind, i, tree, _spp(_scene(kind, i, tree)[2], 5))
    dirs, tan = _rays(oracle, kind, i)
    spp = _spp(_scene(kind, i, tree)[2], 5)
    key = ("denoise", kind, i, tree, tuple(sorted(settings.items())))
    return _once(key, lambda: dr.denoise(frame, _guides(oracle, kind, i, tree), dirs, tan, spp=spp, **{**dr.DEFAULTS, **settings}))


def _upscale_want(oracle, kind, i, tree):
    """(frame, stage) of upscale_ref on the oracle's low frame and guides of both sizes"""
    n = _spp(_scene(kind, i, tree)[2], 3)
    dirs, tan = _rays(oracle, kind, i)
    return _once(("upscale", kind, i, tree), lambda: ur.upscale(_frame(oracle, kind, i, tree, n, low=True), _guides(oracle, kind, i, tree, True),
                                                                _guides(oracle, kind, i, tree), dirs, tan,
                                                                sigma_n=dr.DEFAULTS["sigma_n"], sigma_z=dr.DEFAULTS["sigma_z"]))


def _upscale_want64(oracle, kind, i, tree):
    n = _spp(_scene(kind, i, tree)[2], 3)
    dirs, tan = _rays(oracle, kind, i)
    return _once(("upscale64", kind, i, tree), lambda: ur64.upscale(_frame(oracle, kind, i, tree, n, low=True), _guides(oracle, kind, i, tree, True),
                                                                    _guides(oracle, kind, i, tree), dirs, tan))


def _refine_mask_want(oracle, kind, i, tree):
    b = _scene(kind, i, tree)[0]
    return _once(("refine mask", kind, i, tree), lambda: rr.class_mask(_upscale_want(oracle, kind, i, tree)[1], _guides(oracle, kind, i, tree), b.materials))


def _adaptive_mask_want(oracle, kind, i, tree):
    n = _spp(_scene(kind, i, tree)[2], 3)
    return _once(("adaptive mask", kind, i, tree), lambda: ar.class_mask(_frame(oracle, kind, i, tree, n), _guides(oracle, kind, i, tree),
                                                                       brt.ADAPT_DEFAULT_THRESHOLD, 6))


# ---- CPU: the tables are what they claim; the references alone stay inside the bars ---------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_guides_hit_and_miss_and_hold_no_nan(oracle, kind):
    """Under the scenes' own trees most views see a sphere and the sky; no normal, distance or a of any guide is a NaN (the material
    word of a sky pixel, 0xFFFFFFFF, is no number)."""
    any_hit, both, nan = [], [], []
    for i in range(sc.N_SCENES):
        g = _guides(oracle, kind, i, "ploc")
        hit = g[..., 3] < np.inf
        if hit.any():
            any_hit.append(i)
            if not hit.all():
                both.append(i)
        if np.isnan(g[..., :7]).any():
            nan.append(i)
    print(f"{kind} scenes with a hit: {len(any_hit)}, with hit and miss: {len(both)}, with a NaN in a guide plane: {nan}")
    assert len(any_hit) >= MIN_WITH_A_HIT[kind] and len(both) >= MIN_HIT_AND_MISS[kind] and not nan


@pytest.mark.parametrize("kind", KINDS)
def test_median_split_trees_are_general_and_change_wild_guides(oracle, kind):
    """Every scene of two spheres or more is a GENERAL tree under the median split of three-sphere leaves.  The guides of a sane scene
    do not depend on the tree; those of several wild scenes do (walks cut short by the stack-overflow rule, poisoned boxes, unbounded
    spheres)."""
    differ = []
    for i in range(sc.N_SCENES):
        b = _scene(kind, i, "median3")[0]
        if len(b.models) >= 2:
            assert flavour(b) == "general", (kind, i)
        if not _same(_guides(oracle, kind, i, "ploc"), _guides(oracle, kind, i, "median3")):
            differ.append(i)
    print(f"{kind} scenes whose guides differ between the own tree and median3: {len(differ)} {differ}")
    assert len(differ) >= MIN_TREES_DIFFER[kind] and (kind == "wild" or not differ)


def test_single_leaf_boards_have_one_leaf_of_every_sphere():
    for name in LENS_BOARDS:
        b, _, _, _, w, h = _board(name, "single_leaf")
        assert len(b.bvh) == 1 and b.bvh[0]["model_count"] == len(b.models) >= 64 and w * h >= 64, name
        assert flavour(_board(name, "median3")[0]) == "general", name


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_frames_hold_special_colours_and_filtered_pixels(oracle, kind):
    """The filters' input frames: non-finite colours in the wild table only; most scenes have pixels the filter changes."""
    special, filtered = [], []
    for i in range(sc.N_SCENES):
        cam = _scene(kind, i, "ploc")[2]
        frame = _frame(oracle, kind, i, "ploc", _spp(cam, 5))
        if not np.isfinite(frame[..., :3]).all():
            special.append(i)
        if not dr64.passes_through(frame, _guides(oracle, kind, i, "ploc")).all():
            filtered.append(i)
    print(f"{kind} oracle frames with non-finite colours: {len(special)} {special}; scenes with a filtered pixel: {len(filtered)}")
    assert len(special) >= MIN_NON_FINITE[kind] and (kind == "wild" or not special)
    assert len(filtered) >= MIN_FILTERED[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_denoise_restatement_against_float64(oracle, kind):
    """3 iterations on every scene's own tree: the f32 restatement within the bar of the float64 one on the filtered pixels,
    pass-through pixels equal bit for bit."""
    worst = 0.0
    for i in range(sc.N_SCENES):
        cam = _scene(kind, i, "ploc")[2]
        frame, g = _frame(oracle, kind, i, "ploc", _spp(cam, 5)), _guides(oracle, kind, i, "ploc")
        dirs, tan = _rays(oracle, kind, i)
        f32 = _denoise_want(oracle, kind, i, "ploc", dict(iterations=3))
        f64 = dr64.denoise(frame, g, dirs, tan, spp=_spp(cam, 5), **{**dr.DEFAULTS, "iterations": 3})
        through = dr64.passes_through(frame, g)
        assert _same(f32[through], frame[through]) and _canon_same(f64[through].astype(F32), frame[through]), (kind, i)
        if (~through).any():
            worst = max(worst, _held(f32[~through], f64[~through]))
    print(f"{kind}: denoise f32 restatement against float64, 3 iterations, worst relative error {worst:.3g}")
    assert worst <= BAR


@pytest.mark.parametrize("kind", KINDS)
def test_upscale_restatement_against_float64_and_its_stages(oracle, kind):
    """The f32 restatement within the bar of the float64 one, the stages equal; all three stages and the sky occur."""
    worst, pixels, with_b, with_c = 0.0, {s: 0 for s in (ur.SKY, ur.STAGE_A, ur.STAGE_B, ur.STAGE_C, ur.STAGE_NONE)}, [], []
    for i in range(sc.N_SCENES):
        (f32, stage), (f64, stage64) = _upscale_want(oracle, kind, i, "ploc"), _upscale_want64(oracle, kind, i, "ploc")
        assert np.array_equal(stage, stage64), (kind, i)
        worst = max(worst, _held(f32, f64))
        for s in pixels:
            pixels[s] += int((stage == s).sum())
        if (stage == ur.STAGE_B).any():
            with_b.append(i)
        if (stage == ur.STAGE_C).any():
            with_c.append(i)
    print(f"{kind}: upscale f32 against float64 worst relative error {worst:.3g}; pixels A / B / C / sky / none "
          f"{pixels[ur.STAGE_A]} / {pixels[ur.STAGE_B]} / {pixels[ur.STAGE_C]} / {pixels[ur.SKY]} / {pixels[ur.STAGE_NONE]}; "
          f"scenes with stage B {len(with_b)}, with stage C {len(with_c)}")
    assert worst <= BAR and len(with_b) >= MIN_STAGE_B[kind] and len(with_c) >= MIN_STAGE_C[kind]
    floors = MIN_STAGE_PIXELS[kind]
    for name, s in (("A", ur.STAGE_A), ("B", ur.STAGE_B), ("C", ur.STAGE_C), ("SKY", ur.SKY)):
        assert pixels[s] >= floors[name], (kind, name, pixels[s])


@pytest.mark.parametrize("kind", KINDS)
def test_both_masks_select_some_pixels_and_not_all(oracle, kind):
    adaptive, refine = [], []
    for i in range(sc.N_SCENES):
        m = _adaptive_mask_want(oracle, kind, i, "ploc") != 0
        if m.any() and not m.all():
            adaptive.append(i)
        m = rr.selected(_refine_mask_want(oracle, kind, i, "ploc"), BOTH)
        if m.any() and not m.all():
            refine.append(i)
    print(f"{kind} scenes whose adaptive mask selects some pixels and not all: {len(adaptive)}; whose refine mask does: {len(refine)}")
    assert len(adaptive) >= MIN_ADAPTIVE_MIXED[kind] and len(refine) >= MIN_REFINE_MIXED[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_sphere_ids_have_no_tie(oracle, kind):
    """temporal_ref.sphere_ids recovers every hit's sphere without a tie: no pixel of a temporal state needs to be excused."""
    ties = hits = 0
    for i in range(sc.N_SCENES):
        b, _, cam, _, w, h = _scene(kind, i, "ploc")
        g = _guides(oracle, kind, i, "ploc")
        with np.errstate(all="ignore"):
            _, t = tr.sphere_ids(g, tr.Camera(oracle, cam, w, h), b.models)
        ties += int(t.sum())
        hits += int((g[..., 3] < np.inf).sum())
    print(f"{kind}: temporal_ref.sphere_ids ties {ties} of {hits} hit pixels")
    assert ties == 0 and hits > 20000


@pytest.mark.parametrize("kind", KINDS)
def test_blended_scenes_have_covered_and_uncovered_pixels(oracle, kind):
    blended = [i for i in range(sc.N_SCENES) if _blended(kind, i) is not None]
    own = [i for i in blended if _SCENES[kind]()[i][6] is not None]
    mixed = []
    for i in blended:
        cov = bp.coverage(_coverage_frame(oracle, kind, i, "ploc"))
        if cov.any() and not cov.all():
            mixed.append(i)
    print(f"{kind} scenes of level 1 or 2: {len(blended)} ({len(own)} with own raster inputs); coverage frames with both classes: {len(mixed)}")
    assert len(blended) == MIN_BLENDED[kind] and len(own) == OWN_RASTER[kind] and len(mixed) >= MIN_COVERAGE_MIXED[kind]


# ---- GPU plumbing ---------------------------------------------------------------------------------------------------------------------------

_REFUSED = {}      # (family, kind) -> the scenes whose view the entry point refused
MEASURED = {}      # (family, kind) -> the worst GPU-vs-restatement error seen (printed by the tests)


def _refusal(family, kind, i, error):
    """A view the entry point refuses by a documented rule: an invalid argument or an unsupported one, with its text."""
    assert error.code in (-1, -8) and error.text, (family, kind, i, error)
    _REFUSED.setdefault((family, kind), set()).add(i)
    assert len(_REFUSED[family, kind]) <= MAX_REFUSED, (family, kind, sorted(_REFUSED[family, kind]))


def _worst(family, kind, err):
    MEASURED[family, kind] = max(MEASURED.get((family, kind), 0.0), err)


def _report(family, kind):
    print(f"{family}, {kind}: worst error {MEASURED.get((family, kind), 0.0):.3g}, refused {sorted(_REFUSED.get((family, kind), ()))}")


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the oracle's arrays are shared and read-only)


def _out(w, h, fmt=brt.FLAG_OUT_RGBA32F):
    import torch
    return torch.zeros((h, w * brt.OUT_PIXEL_BYTES[fmt] // 4), dtype=torch.int32, device="cuda")


def _host(t, h, w, fmt=brt.FLAG_OUT_RGBA32F):
    import torch
    torch.cuda.synchronize()
    raw = t.cpu().numpy()
    return raw.view(F32).reshape(h, w, 4) if fmt == brt.FLAG_OUT_RGBA32F else raw.view(np.uint8).reshape(h, w, -1)


def _packed(oracle, f32, name):
    e = np.ascontiguousarray(oracle.encode_frame(f32, name))
    return e.view(np.uint8).reshape(f32.shape[0], f32.shape[1], -1)


def _what(kind, i, tree):
    b, _, cam, _, w, h = _scene(kind, i, tree)
    return f"{kind} case {i} under {tree}: {len(b.models)} spheres, {len(b.bvh)} nodes, {w}x{h}"


# ---- GPU 1: the guides, bitwise ---------------------------------------------------------------------------------------------------------------

def _assert_guides(got, want, what):
    bad = (_canon(got) != _canon(want)).any(axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} guide pixels differ, first {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
@pytest.mark.parametrize("kind", KINDS)
def test_guides_on_randomized_and_wild_scenes(plugin, oracle, kind, tree):
    """brt_debug_denoise_guides at both sizes of every scene: normal, t, a and the material word are the oracle's raycast on the tree
    the GPU walked with the material table's rule for a (refracting: 1, else sqrt(max(base, 1e-3))) -- fractional, negative, NaN and
    INF transmissions, base colours outside [0, 1], multi-sphere leaves, walks the overflow rule cuts short."""
    hits = 0
    for i in range(sc.N_SCENES):
        b, _, cam, win, w, h = _scene(kind, i, tree)
        plugin.node.write_buffers(b)
        for low in (False, True):
            sw, sh, swin = _size_window(kind, i, low)
            try:
                got = plugin.debug_denoise_guides(cam, swin, sw, sh)
            except brt.BrtError as e:
                _refusal("guides", kind, i, e)
                break
            _assert_guides(got, _guides(oracle, kind, i, tree, low), f"{_what(kind, i, tree)}, {'low' if low else 'full'} size")
            hits += int((got[..., 3] < np.inf).sum())
    _report("guides", kind)
    assert hits > 20000


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["single_leaf", "median3"])
def test_guides_on_the_boards(plugin, oracle, tree):
    """The lane boards under one leaf of every sphere and under three-sphere leaves: pixel k carries material k, the leaf's last
    sphere included; every plane is the oracle's."""
    for name in LENS_BOARDS:
        b, _, cam, win, w, h = _board(name, tree)
        plugin.node.write_buffers(b)
        got = plugin.debug_denoise_guides(cam, win, w, h)
        _assert_guides(got, dr.guides(oracle, b, cam, w, h, window=win), f"{name} under {tree}")
        assert np.array_equal(np.ascontiguousarray(got[..., 7]).view(U32).reshape(-1), np.arange(w * h)), (name, tree)


# ---- GPU 2: denoise ------------------------------------------------------------------------------------------------------------------------------

def _denoise_dev(plugin, cam, win, w, h, frame, fmt=brt.FLAG_OUT_RGBA32F, flags=0):
    d_in, out = _dev(frame), _out(w, h, fmt)
    plugin.node.denoise_device(cam, win, w, h, d_in.data_ptr(), out.data_ptr(), out_format=fmt, flags=flags)
    return _host(out, h, w, fmt)


def _check_filtered(got, want, frame, through, family, kind, what):
    """Pass-through pixels are their input bit for bit (alpha with them); filtered pixels are inside the bar."""
    assert _same(got[through], frame[through]), f"{what}: a pass-through pixel changed"          # (copies: a NaN keeps its sign and payload)
    assert _same(got[..., 3], frame[..., 3]), f"{what}: alpha changed"
    if (~through).any():
        err = _held(got[~through], want[~through])
        _worst(family, kind, err)
        assert err <= BAR, (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
@pytest.mark.parametrize("kind", KINDS)
def test_denoise_on_randomized_and_wild_scenes(plugin, oracle, kind, tree):
    """brt_denoise_device on the oracle's frame, iterations 1, 3, 5 rotating over the scenes, every eighth scene also under another
    sigma set; the first three scenes with filtered pixels through one packed format each."""
    t = SCENE_TREES.index(tree)
    packed = list(PACKED)
    try:
        for i in range(sc.N_SCENES):
            b, _, cam, win, w, h = _scene(kind, i, tree)
            cam = _at(cam, _spp(cam, 5))
            frame = _frame(oracle, kind, i, tree, _spp(cam, 5))
            through = dr64.passes_through(frame, _guides(oracle, kind, i, tree))
            plugin.node.write_buffers(b)
            runs = [dict(iterations=ITERATIONS[(i + t) % 3])] + ([OTHER_SIGMAS] if i % 8 == t else [])
            for s in runs:
                full = {**dr.DEFAULTS, **s}
                plugin.set_denoise(full["iterations"], full["sigma_l"], full["sigma_n"], full["sigma_z"])
                try:
                    got = _denoise_dev(plugin, cam, win, w, h, frame)
                except brt.BrtError as e:
                    _refusal("denoise", kind, i, e)
                    break
                _check_filtered(got, _denoise_want(oracle, kind, i, tree, s), frame, through, "denoise", kind, f"{_what(kind, i, tree)}, {s}")
                if packed and s is runs[0] and (~through).any():
                    fmt, name = packed.pop(0)
                    assert _same(_denoise_dev(plugin, cam, win, w, h, frame, fmt), _packed(oracle, got, name)), (_what(kind, i, tree), name)
    finally:
        plugin.set_denoise()
    _report("denoise", kind)
    assert not packed


# ---- GPU 3: blend-post (k_denoise_guides_cov) -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
@pytest.mark.parametrize("kind", KINDS)
def test_blend_post_on_the_blended_scenes(plugin, oracle, kind, tree):
    """The level-1/2 scenes: the oracle's coverage frame through brt_blend_post_device in the DENOISE mode.  Covered pixels are their
    raster texels bit for bit, the others are held to blend_post_ref.denoise_frame."""
    plugin.set_denoise()
    ran = 0
    for i in range(sc.N_SCENES):
        if _blended(kind, i) is None:
            continue
        b, _, cam, win, w, h = _scene(kind, i, tree)
        cam = _at(cam, _spp(cam, 5))
        rgba = _blended(kind, i)[0]
        covf = _coverage_frame(oracle, kind, i, tree)
        cov = bp.coverage(covf)
        plugin.node.write_buffers(b)
        d_cov, d_rgba, out = _dev(covf), _dev(rgba), _out(w, h)
        try:
            plugin.node.blend_post_device(cam, win, w, h, d_cov.data_ptr(), out.data_ptr(), d_rgba.data_ptr(), flags=brt.FLAG_DENOISE)
        except brt.BrtError as e:
            _refusal("blend post", kind, i, e)
            continue
        got = _host(out, h, w)
        what = _what(kind, i, tree)
        assert _same(got[cov], rgba[cov]), f"{what}: a covered pixel is not its raster texel"
        g = _guides(oracle, kind, i, tree)
        want = bp.denoise_frame(oracle, covf, g, cam, rgba)
        through = dr64.passes_through(covf, bp.cover_guides(g, cov))              # (a covered pixel is a miss: it passes through)
        assert _same(got[through & ~cov], covf[through & ~cov]), f"{what}: an uncovered pass-through pixel changed"
        if (~through).any():
            err = _held(got[~through], want[~through])
            _worst("blend post", kind, err)
            assert err <= BAR, (what, err)
        ran += 1
    _report("blend post", kind)
    assert ran >= MIN_BLENDED[kind] - MAX_REFUSED


# ---- GPU 4: upscale, its blended pack, the select pack and the refined frame ----------------------------------------------------------------------

def _check_upscaled(got, want, want64, stage, family, kind, what):
    """Sky pixels and pixels of no stage bit for bit, stages A, B, C inside the bar of both restatements."""
    exact = (stage == ur.SKY) | (stage == ur.STAGE_NONE)
    assert _canon_same(got[exact], want[exact]), f"{what}: a sky pixel or a pixel of no stage differs"
    assert _canon_same(got[..., 3], want[..., 3]), f"{what}: alpha differs"
    if (~exact).any():
        e32, e64 = _held(got[~exact], want[~exact]), _held(got[~exact], want64[~exact])
        _worst(family, kind, e32)
        _worst(family + " (float64)", kind, e64)
        assert e32 <= BAR and e64 <= BAR, (what, e32, e64)


@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
@pytest.mark.parametrize("kind", KINDS)
def test_upscale_on_randomized_and_wild_scenes(plugin, oracle, kind, tree):
    """brt_upscale_device on the oracle's low frame: k_upscale's own walk of every output pixel's guide on general trees, the tap
    eligibility from the low guides.  The level-1/2 scenes also through brt_upscale_blend_device against upscale_blend_ref."""
    blended = 0
    for i in range(sc.N_SCENES):
        b, lvl, cam, win, w, h = _scene(kind, i, tree)
        lw, lh, _ = _low(kind, i)
        cam = _at(cam, _spp(cam, 3))
        low = _frame(oracle, kind, i, tree, _spp(cam, 3), low=True)
        (want, stage), (want64, _) = _upscale_want(oracle, kind, i, tree), _upscale_want64(oracle, kind, i, tree)
        plugin.node.write_buffers(b)
        d_low, out = _dev(low), _out(w, h)
        what = _what(kind, i, tree)
        try:
            plugin.node.upscale_device(cam, win, lw, lh, d_low.data_ptr(), w, h, out.data_ptr())
        except brt.BrtError as e:
            _refusal("upscale", kind, i, e)
            continue
        _check_upscaled(_host(out, h, w), want, want64, stage, "upscale", kind, what)
        if _blended(kind, i) is None:
            continue
        rgba, depth = _blended(kind, i)
        dirs, tan = _rays(oracle, kind, i)
        want_b, stage_b = ubr.upscale(low, _guides(oracle, kind, i, tree, True), _guides(oracle, kind, i, tree), dirs, tan, cam,
                                      int(lvl["level"][0]), rgba, depth, sigma_n=dr.DEFAULTS["sigma_n"], sigma_z=dr.DEFAULTS["sigma_z"])
        d_rgba, d_depth, out = _dev(rgba), _dev(depth), _out(w, h)
        try:
            plugin.node.upscale_blend_device(lvl, cam, win, lw, lh, d_low.data_ptr(), w, h, out.data_ptr(), d_rgba.data_ptr(), d_depth.data_ptr())
        except brt.BrtError as e:
            _refusal("upscale blend", kind, i, e)
            continue
        got = _host(out, h, w)
        cov = stage_b == ubr.COVERED
        assert _same(got[cov], rgba[cov]), f"{what}: a covered pixel is not its raster texel"
        keep = ~cov
        assert _canon_same(want_b[keep], want[keep])                               # (the blended restatement is upscale_ref's there)
        _check_upscaled(np.where(keep[..., None], got, want), want, want64, stage, "upscale blend", kind, what)
        blended += 1
    for family in ("upscale", "upscale (float64)", "upscale blend"):
        _report(family, kind)
    assert blended >= MIN_BLENDED[kind] - MAX_REFUSED


def _tuned(plugin, run):
    """The re-trace of the selected pixels under a residency of the streaming form, or in the plain form."""
    return plugin.tuning(BRT_PIXELS_FORM=1) if run == "plain" else plugin.tuning(**RESIDENCIES[run][0])


@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
@pytest.mark.parametrize("kind", KINDS)
def test_refined_upscale_on_randomized_and_wild_scenes(plugin, oracle, kind, tree):
    """brt_upscale_refine_mask_device is upscale_refine_ref.class_mask exactly; brt_upscale_refine_device selects that set, counts it,
    and every selected pixel is the oracle's full-size pixel bit for bit, the others are brt_upscale_device's."""
    import torch
    t = SCENE_TREES.index(tree)
    selected = 0
    for i in range(sc.N_SCENES):
        b, _, cam, win, w, h = _scene(kind, i, tree)
        lw, lh, _ = _low(kind, i)
        n = _spp(cam, 3)
        cam = _at(cam, n)
        low = _frame(oracle, kind, i, tree, n, low=True)
        want_mask = _refine_mask_want(oracle, kind, i, tree)
        what = _what(kind, i, tree)
        plugin.node.write_buffers(b)
        d_low = _dev(low)
        mask = torch.full((h, w), 0x55, dtype=torch.uint8, device="cuda")
        try:
            plugin.node.upscale_refine_mask_device(cam, win, lw, lh, d_low.data_ptr(), w, h, mask.data_ptr())
        except brt.BrtError as e:
            _refusal("refine", kind, i, e)
            continue
        torch.cuda.synchronize()
        got_mask = mask.cpu().numpy()
        assert np.array_equal(got_mask, want_mask), f"{what}: {int((got_mask != want_mask).sum())} class bytes differ"
        up, out = _out(w, h), _out(w, h)
        plugin.node.upscale_device(cam, win, lw, lh, d_low.data_ptr(), w, h, up.data_ptr())
        up = _host(up, h, w)
        full = _frame(oracle, kind, i, tree, n)
        classes = (BOTH, brt.REFINE_EDGES, brt.REFINE_SPECULAR)[(i + t) % 3]
        sel = rr.selected(want_mask, classes)
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        with _tuned(plugin, RETRACE_RUNS[(i + t) % 4]):
            plugin.node.upscale_refine_device(cam, win, lw, lh, d_low.data_ptr(), w, h, out.data_ptr(), classes, count.data_ptr())
        got = _host(out, h, w)
        assert int(count.cpu()[0]) == int(sel.sum()), (what, classes)
        assert _canon_same(got[sel], full[sel]), f"{what}: a selected pixel is not the oracle's full-size pixel"
        assert _same(got[~sel], up[~sel]), f"{what}: an unselected pixel is not brt_upscale_device's"
        selected += int(sel.sum())
    _report("refine", kind)
    assert selected > 1000


# ---- GPU 5: adaptive -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_on_randomized_and_wild_scenes(plugin, oracle, kind, tree):
    """brt_adaptive_mask_device on the oracle's base frame is adaptive_ref.class_mask exactly (default threshold, min_taps 6);
    brt_adaptive_refine_device is the base frame with the selected pixels replaced by the oracle's at two samples more, bit for bit,
    with their count."""
    import torch
    t = SCENE_TREES.index(tree)
    selected = 0
    try:
        for i in range(sc.N_SCENES):
            b, _, cam, win, w, h = _scene(kind, i, tree)
            n = _spp(cam, 3)
            cam = _at(cam, n + ADAPT_MORE)
            base, full = _frame(oracle, kind, i, tree, n), _frame(oracle, kind, i, tree, n + ADAPT_MORE)
            want_mask = _adaptive_mask_want(oracle, kind, i, tree)
            what = _what(kind, i, tree)
            plugin.node.write_buffers(b)
            plugin.set_adaptive(n, brt.ADAPT_DEFAULT_THRESHOLD, 6)
            d_base = _dev(base)
            mask = torch.full((h, w), 0x55, dtype=torch.uint8, device="cuda")
            try:
                plugin.node.adaptive_mask_device(cam, win, w, h, d_base.data_ptr(), mask.data_ptr())
            except brt.BrtError as e:
                _refusal("adaptive", kind, i, e)
                continue
            torch.cuda.synchronize()
            got_mask = mask.cpu().numpy()
            assert np.array_equal(got_mask, want_mask), f"{what}: {int((got_mask != want_mask).sum())} class bytes differ"
            out = _out(w, h)
            count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            with _tuned(plugin, RETRACE_RUNS[(i + t + 1) % 4]):
                plugin.node.adaptive_refine_device(cam, win, w, h, d_base.data_ptr(), out.data_ptr(), count.data_ptr())
            got = _host(out, h, w)
            assert int(count.cpu()[0]) == int((want_mask != 0).sum()), what
            sel = want_mask != 0
            assert _same(got[~sel], base[~sel]), f"{what}: an unselected pixel is not the base frame's, byte for byte"
            assert _canon_same(got[sel], full[sel]), f"{what}: a selected pixel is not the oracle's at the camera's samples"
            assert _canon_same(got, ar.adaptive(base, full, want_mask)), what
            selected += int((want_mask != 0).sum())
    finally:
        plugin.set_adaptive()
    _report("adaptive", kind)
    assert selected > 1000


# ---- GPU 6: temporal ---------------------------------------------------------------------------------------------------------------------------------

MOVE = np.array([0.03, -0.02, 0.025], F32)                  # |MOVE| < 0.1, the pad of a leaf box (Model::aabb): the tree's bytes stay valid


def _moved(oracle, i, tree):
    """The scene with every third sphere the view hits moved by MOVE, under the same tree bytes."""
    b = _scene("random", i, tree)[0]
    g = _guides(oracle, "random", i, tree)
    cam, _, w, h = _scene("random", i, tree)[2:]
    with np.errstate(all="ignore"):
        sid, _ = tr.sphere_ids(g, tr.Camera(oracle, cam, w, h), b.models)
    hit_ids = np.unique(sid[g[..., 3] < np.inf])
    models = b.models.copy()
    models["position"][hit_ids[::3]] += MOVE
    return brt.Buffers(models, b.materials, b.bvh), hit_ids[::3]


def _temporal_sequence(plugin, oracle, i, tree, denoise_on):
    """Three frames of scene i through brt_denoise_device with FLAG_TEMPORAL: still, still with another window seed, then an upload
    with moved spheres.  The input frames are the oracle's; state and frame against temporal_ref after every step.
    -> [(frame, state)], or None where the entry point refuses the view."""
    b, lvl, cam, win, w, h = _scene("random", i, tree)
    n = _spp(cam, 5)
    cam = _at(cam, n)
    flags = brt.FLAG_TEMPORAL | (brt.FLAG_DENOISE if denoise_on else 0)
    win2 = win.copy()
    win2["random_seed"] = F32(win[0]["random_seed"]) * F32(0.5) + F32(0.3)
    moved, picked = _moved(oracle, i, tree)
    c = tr.Camera(oracle, cam, w, h)
    hist = tr.History()
    plugin.set_temporal()
    plugin.set_denoise()
    out = []
    for step, (buffers, window) in enumerate(((b, win), (b, win2), (moved, win2))):
        if step != 1:
            plugin.node.write_buffers(buffers)
        if step == 0:
            plugin.reset_temporal()
        frame = np.asarray(oracle.render(buffers, _pure(lvl), cam, window, w, h)[0], F32)
        g = _guides(oracle, "random", i, tree) if buffers is b else dr.guides(oracle, buffers, cam, w, h, window=window)
        with np.errstate(all="ignore"):
            sid, ties = tr.sphere_ids(g, c, buffers.models)
        assert not ties.any(), ("random", i, tree, step)
        want = tr.frame_step(hist, frame, g, sid, c, tr.spheres_of(buffers.models), n, denoise_on)
        try:
            got = _denoise_dev(plugin, cam, window, w, h, frame, flags=flags)
        except brt.BrtError as e:
            _refusal("temporal", "random", i, e)
            return None
        state = plugin.debug_temporal_state(w, h)
        what = f"{_what('random', i, tree)}, frame {step}, {'temporal | denoise' if denoise_on else 'temporal'}"
        _compare_state(state, tr.state(hist), np.ones((h, w), bool))
        err = _rel(got, want)
        _worst("temporal", "random", err)
        assert err <= BAR, (what, err)
        out.append((got, state))
    return out, int(picked.size), int((out[-1][1][..., 3] >= 2).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
def test_temporal_sequences_on_the_randomized_scenes(plugin, oracle, tree):
    """FLAG_TEMPORAL and FLAG_TEMPORAL | FLAG_DENOISE alternating over the scenes: sid through the guide kernel on multi-sphere leaves,
    the motion term on moved spheres under the caller's tree, n and the rejections exact, x', y' within 1e-4 px, no pixel excused."""
    t = SCENE_TREES.index(tree)
    moved = kept = 0
    try:
        for i in range(sc.N_SCENES):
            res = _temporal_sequence(plugin, oracle, i, tree, (i + t) % 2 == 1)
            if res is not None:
                moved += res[1]
                kept += res[2]
    finally:
        plugin.set_temporal()
        plugin.set_denoise()
    _report("temporal", "random")
    print(f"temporal under {tree}: {moved} spheres moved, {kept} pixels keep a history through the last frame")
    assert moved >= 150 and kept >= 20000                         # (measured: 169 and 24 263 under either tree)


HOT_SIZE, HOT_SPP = (96, 54), 64


@pytest.mark.gpu
def test_no_hot_order_on_a_general_tree():
    """prepass_order counts record visits, and apply_hot_order then renumbers records and spheres, only for a scene of 16-bit
    descriptors, a SIMPLE tree and more than 64 pair records that is walked from the LDS tile (brt_api_order.cpp).  The 10 004-sphere
    grid meets every condition but the tree's: under the median split of three-sphere leaves the first 64-sample frame of a fresh
    context runs its pre-pass with the top of the tree in LDS and renumbers nothing, and neither do the frames behind it -- so rmap
    is null in the guide kernel on every general tree.  The control, the same spheres and view under the callee's tree in another
    fresh context, is renumbered by its first frame."""
    from helpers import median_split_bvh
    b = brt.generate_scene(brt.SCENE_STRESS_GRID, 1)
    w, h = HOT_SIZE
    general = brt.Buffers(b.models, b.materials, median_split_bvh(b.models, 3))
    assert general.bvh["model_count"].max() == 3 and int((general.bvh["model_count"] == 0).sum()) > 64 and len(b.models) <= 16382
    seen = []
    with brt.RaytracePlugin([0]) as p:
        for k, seed in enumerate((0.5, 0.25, 0.75)):
            lvl, cam, win = brt.cover_camera(w, h, HOT_SPP, 1, brt.Raytracing.Pure, seed)
            p.node.run(lvl, cam, win, w, h, buffers=general if k == 0 else None)
            seen.append(dict(p.node.last_stats))
    print("general tree:", [(st["scene_in_lds"], st["hot_records"], st["prepass_ms"] > 0.0) for st in seen])
    assert seen[0]["prepass_ms"] > 0.0, seen[0]
    assert all(st["scene_in_lds"] == 2 and st["hot_records"] == 0 for st in seen), seen
    with brt.RaytracePlugin([0]) as p:
        lvl, cam, win = brt.cover_camera(w, h, HOT_SPP, 1, brt.Raytracing.Pure, 0.5)
        p.node.run(lvl, cam, win, w, h, buffers=brt.Buffers(b.models, b.materials, None))
        control = dict(p.node.last_stats)
    print("callee's tree:", control["scene_in_lds"], control["hot_records"], control["prepass_ms"] > 0.0)
    assert control["scene_in_lds"] == 2 and control["prepass_ms"] > 0.0 and control["hot_records"] > 64, control
