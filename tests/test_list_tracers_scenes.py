"""The list tracers -- k_list_plain and k_list_stream<Start, MODE, D16, SIMPLE> of brt_pixels_dev.h, under PinholeStart and the thin-lens and
orthographic LensStart -- on general trees and hostile scenes: the randomized and wild scenes and the boards of tests/shade_cases.py, bit
for bit against the C oracle.  (tests/test_pixels.py and tests/test_lens.py render simple trees only.)

  * CPU: the case table is what it claims.  Every scene's walk flavour is recomputed from its tree by the rule of validate_and_encode
    (brt_host.cpp: single-sphere leaves and max leaf depth + 1 < 31 are a SIMPLE tree, all else a GENERAL one); the wild scenes that clear
    boxes_ordered or spheres_bounded are counted; the boards keep their claim -- every pixel's first sample meets its own sphere -- under a
    median-split tree of three-sphere leaves and under one leaf of every sphere; the lens views of the randomized scenes hit something.
  * GPU, pinhole lists: every randomized and wild scene with its own camera, window, sample and bounce count.  The list names every pixel
    once in a shuffled order, a third as many repeats at random places and refused entries at places 0, 31, 32, 63 and 64; streaming form
    under three residencies, plain form, host entry point.
  * GPU, boards: every case of shade_cases.PURE under its PLOC tree, the median-split tree and the single-leaf tree.  In a list kernel
    the lane of a pixel is its place in the list: list (a) puts pixel k at place lane_of(k, w), so that lane l of the first wave holds what
    lane l of the frame kernel's tile held; (b) is (a) backwards; (c) five copies of the pixels shuffled together.
  * GPU, lens rules at one sample: all randomized scenes and eight boards (PLOC and median-split tree), every pixel's ray and RNG state
    from brt.lens_ray and its colour from oracle.radiance on the tree the GPU walked; at several samples two general-tree scenes
    against the numpy restatement (lens_ref.pixel).
  * The table of instantiations that ran, asserted per cell at the end.

The lens numbers.  Randomized scenes keep their own camera and window: the thin lens has aperture radius 0.25 and is focused at the
camera's distance from the origin; the orthographic view has ortho_height 8.  (Measured on the oracle: 35 thin-lens and 35 orthographic
views of the 40 cast more rays than paths -- all whose scene has a bounce at all; the test prints both.)  A board's camera sits AT the origin, where that focus distance would
be 0, which the lens entry points refuse: a board's thin lens is focused at the spheres' distance (shade_cases.DISTANCE) and its
orthographic view is as high as the perspective view is at that distance, 2 * DISTANCE * tan(FOV / 2), so that the lanes still meet
their own spheres.

Every comparison is an equality of bits; a NaN equals a NaN at the same place."""
import functools
import math

import numpy as np
import pytest

import bevyray_amd as brt
import lens_ref as lr
import query_ref as qr
import shade_cases as sc
from helpers import dev, guarded, median_split_bvh, single_leaf_bvh
from test_lens import _one_sample_frame, _ortho, _twin_rays

npr = lr.npr
F32 = np.float32
GUARD, FILL = 256, 0xCD
PIXELS_STREAM, PIXELS_PLAIN, LENS_STREAM, LENS_PLAIN = 32, 33, 34, 35      # brt_stats::kernel_variant
# name -> (knobs, the scene_in_lds a streaming launch must report): every scene here fits the LDS of one workgroup
RESIDENCIES = {"lds": ({}, 1), "lds_top": ({"BRT_FORCE_LDS_TOP": 5}, 2), "global": ({"BRT_FORCE_GLOBAL_SCENE": 1}, 0)}
PLACEMENT = {1: "LDS", 2: "LDS_TOP", 0: "GLOBAL"}
REFUSED_PLACES = (0, 31, 32, 63, 64)
THIN_APERTURE, ORTHO_HEIGHT = 0.25, 8.0
BOARD_ORTHO_HEIGHT = 2.0 * sc.DISTANCE * math.tan(sc.FOV / 2.0)
MIN_PER_FLAVOUR = 15          # general and simple scenes per table
MIN_LENS_VIEWS = 20           # lens views per rule that hit something
MIN_LAUNCHES = 10             # per cell of the table of instantiations


# ---- trees ---------------------------------------------------------------------------------------------------------------------------------

def _reachable(bvh):
    """node -> depth of the nodes the root reaches"""
    depth, frontier = {0: 0}, [0]
    while frontier:
        n = frontier.pop()
        if bvh[n]["model_count"] == 0:
            for c in (int(bvh[n]["index"]), int(bvh[n]["index"]) + 1):
                depth[c] = depth[n] + 1
                frontier.append(c)
    return depth


def flavour(b):
    """"simple" or "general" by the rule of brt_host.cpp (e.simple_tree): every leaf holds one sphere and validate_scene's depth + 1 < 31."""
    depth = brt.validate_scene(b.models, b.materials, b.bvh)
    reach = _reachable(b.bvh)
    assert depth == max(d for n, d in reach.items() if b.bvh[n]["model_count"] > 0)
    one = all(b.bvh[n]["model_count"] == 1 for n in reach if b.bvh[n]["model_count"] > 0)
    return "simple" if one and depth + 1 < 31 else "general"


def boxes_ordered(bvh):
    """brt_host.cpp: every child box of a reachable interior node is finite with min <= max."""
    for n in _reachable(bvh):
        if bvh[n]["model_count"] == 0:
            for c in (int(bvh[n]["index"]), int(bvh[n]["index"]) + 1):
                lo, hi = bvh[c]["bounds_min"], bvh[c]["bounds_max"]
                if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
                    return False
    return True


def spheres_bounded(models):
    """brt_layout.h: every |centre_i| <= kLeafCentreMax = 2^24 and r * r (f32) <= kLeafR2Max = 2^50; a NaN fails."""
    with np.errstate(all="ignore"):
        r2 = models["radius"].astype(F32) * models["radius"].astype(F32)
        return bool((np.abs(models["position"].astype(F32)) <= F32(2.0 ** 24)).all() and (r2 <= F32(2.0 ** 50)).all())


TREES = {"ploc": lambda b: b, "median3": lambda b: brt.Buffers(b.models, b.materials, median_split_bvh(b.models, 3)),
         "single_leaf": lambda b: brt.Buffers(b.models, b.materials, single_leaf_bvh(b.models))}
_SCENES = {"random": sc.random_scenes, "wild": sc.wild_scenes}
_FLAVOUR = {}


def _flavour_of(key, b):
    if key not in _FLAVOUR:
        _FLAVOUR[key] = flavour(b)
    return _FLAVOUR[key]


@functools.lru_cache(maxsize=None)
def _board(name, tree):
    """The case `name` of shade_cases.PURE with its spheres and materials under another tree -> (buffers, level, camera, window, w, h)"""
    b, lvl, cam, win, w, h, knobs = sc.PURE[name]()
    assert knobs == {}
    return TREES[tree](b), lvl, cam, win, w, h


# ---- the lists -----------------------------------------------------------------------------------------------------------------------------

def _refused_value(j, n_px):
    return (n_px, n_px + 1, 0xFFFFFFFF)[j % 3]


def _with_refused(lst, n_px):
    """Refused entries at places 0, 31, 32, 63 and 64 where the list is that long"""
    for j, place in enumerate(REFUSED_PLACES):
        if place <= lst.size:
            lst = np.insert(lst, place, _refused_value(j, n_px))
    return lst.astype(np.uint32)


def scene_list(w, h, seed, repeats=True):
    """Every pixel once in a shuffled order, w * h // 3 repeats at random places, the refused entries."""
    rng = np.random.default_rng(seed)
    n = w * h
    lst = rng.permutation(n).astype(np.int64)
    if repeats and n >= 3:
        lst = np.insert(lst, rng.integers(0, n + 1, n // 3), rng.integers(0, n, n // 3))
    return _with_refused(lst, n)


def board_lists(w, h, seed):
    """(a) pixel k at place lane_of(k, w), the places between refused; (b) the same backwards; (c) five copies shuffled together."""
    n = w * h
    a = np.array([_refused_value(j, n) for j in range(sc.lane_of(n - 1, w) + 1)], np.uint32)
    for k in range(n):
        a[sc.lane_of(k, w)] = k
    c = np.random.default_rng(seed).permutation(np.tile(np.arange(n, dtype=np.uint32), 5))
    return {"a": a, "b": a[::-1].copy(), "c": c}


def test_the_lists_are_what_they_claim():
    for w, h in ((1, 1), (5, 7), (8, 8), (69, 47)):
        n = w * h
        lst = scene_list(w, h, 7)
        ok = lst < n
        assert np.array_equal(np.unique(lst[ok]), np.arange(n)) and ok.sum() == n + (n // 3 if n >= 3 else 0)
        bad = [p for p in REFUSED_PLACES if p < lst.size and not ok[p]]
        assert (~ok).sum() == len(bad) and len(bad) == sum(1 for j, p in enumerate(REFUSED_PLACES) if p <= n + (n // 3 if n >= 3 else 0) + j), (w, h, bad)
        assert set(lst[~ok].tolist()) <= {n, n + 1, 0xFFFFFFFF}
    assert len({tuple(scene_list(8, 8, s)) for s in range(4)}) == 4
    for w, h in sc.SMALL_SIZES:
        ls = board_lists(w, h, 3)
        a = ls["a"]
        assert all(a[sc.lane_of(k, w)] == k for k in range(w * h)) and (a < w * h).sum() == w * h and a.size == (h - 1) * 8 + w
        assert np.array_equal(ls["b"], a[::-1]) and np.array_equal(np.sort(ls["c"]), np.repeat(np.arange(w * h), 5))
    assert board_lists(8, 8, 3)["c"].size == 320 and np.array_equal(board_lists(8, 8, 3)["a"], np.arange(64))


# ---- CPU: the case table is what it claims -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(_SCENES))
def test_simple_and_general_scenes(kind):
    """At least 15 general and 15 simple trees among the 40 scenes of each table; the library refuses none."""
    scenes = _SCENES[kind]()
    tally = {"simple": [], "general": []}
    for i, case in enumerate(scenes):
        tally[_flavour_of((kind, i), case[0])].append(i)
    print(f"{kind} scenes: {len(tally['general'])} general {tally['general']}, {len(tally['simple'])} simple {tally['simple']}")
    assert len(scenes) == sc.N_SCENES
    assert len(tally["general"]) >= MIN_PER_FLAVOUR and len(tally["simple"]) >= MIN_PER_FLAVOUR, tally


def test_wild_scenes_clear_the_walk_flags():
    """Scenes whose upload clears boxes_ordered (a non-finite or inverted child box) or spheres_bounded (a centre beyond 2^24, r^2
    beyond 2^50, a NaN): walk_run then leaves the hand-written leaf step, or the hand-written loops, at run time.  At least one of each."""
    scenes = sc.wild_scenes()
    unordered = [i for i, case in enumerate(scenes) if not boxes_ordered(case[0].bvh)]
    unbounded = [i for i, case in enumerate(scenes) if not spheres_bounded(case[0].models)]
    traced = lambda idx: [i for i in idx if int(scenes[i][2][0]["sample_count"]) > 0]
    print(f"wild scenes that clear boxes_ordered: {unordered} (with samples: {traced(unordered)}); spheres_bounded: {unbounded} (with samples: {traced(unbounded)})")
    assert len(traced(unordered)) >= 1 and len(traced(unbounded)) >= 1
    assert all(boxes_ordered(case[0].bvh) and spheres_bounded(case[0].models) for case in sc.random_scenes())      # (the rule is not trivially false)


def _first_hit_materials(oracle, b, cam, win, w, h):
    o, d, _ = oracle.first_sample_rays(cam, win, w, h)
    return qr.expected(oracle, b.models, b.bvh, qr.make_rays(o, d))[0]["material"]


@pytest.mark.parametrize("name", list(sc.PURE))
def test_boards_keep_their_claim_under_general_trees(oracle, name):
    """Same spheres and materials, another tree: the first-sample ray of pixel k meets the sphere of material k (no sphere: the sky,
    on these open boards) in the PLOC tree, the median-split tree of three-sphere leaves and the single leaf; both hand-made trees are
    GENERAL ones wherever the board has two spheres."""
    b, _, cam, win, w, h = _board(name, "ploc")
    present = set(b.models["material_id"].tolist())
    want = [k if k in present else brt.QUERY_NONE for k in range(w * h)]
    for tree in TREES:
        bt = _board(name, tree)[0]
        assert _first_hit_materials(oracle, bt, cam, win, w, h).tolist() == want, (name, tree)
        want_flavour = "simple" if tree == "ploc" or len(b.models) < 2 else "general"
        assert _flavour_of(("board", name, tree), bt) == want_flavour, (name, tree)


def _lens_view(kind, cam, lens_rule):
    """-> (camera at one sample, lens) of a rule for a scene of the randomized table or a board"""
    c = (_ortho(cam) if lens_rule == "ortho" else cam).copy()
    c["sample_count"] = 1
    if kind == "board":
        return c, (brt.lens(0.0, 1.0, BOARD_ORTHO_HEIGHT) if lens_rule == "ortho" else brt.lens(THIN_APERTURE, sc.DISTANCE))
    focus = float(np.linalg.norm(cam[0]["position"].astype(np.float64)))
    return c, (brt.lens(0.0, 1.0, ORTHO_HEIGHT) if lens_rule == "ortho" else brt.lens(THIN_APERTURE, focus))


LENS_BOARDS = ("lottery_open", "lottery_enclosed", "ladder2_open", "ladder2_enclosed", "glass_open", "colours_open", "pat_d_even_m_odd_b6",
               "pat_d31_m32_rest_g_b6")
LENS_CASES = [("random", i, "own") for i in range(sc.N_SCENES)] + [("board", name, tree) for name in LENS_BOARDS for tree in ("ploc", "median3")]
_LENS_WANT = {}


def _lens_scene(kind, which, tree):
    if kind == "board":
        return _board(which, tree)
    return sc.random_scenes()[which][:6]


def _lens_want(oracle, kind, which, tree, lens_rule):
    """(camera, lens, (n, 4) f32 frame of the twin's rays shaded by the oracle at one sample, rays cast), once"""
    key = (kind, which, tree, lens_rule)
    if key not in _LENS_WANT:
        b, _, cam, win, w, h = _lens_scene(kind, which, tree)
        c, lens = _lens_view(kind, cam, lens_rule)
        want, n_rays = _one_sample_frame(oracle, b, _twin_rays(c, win, lens, w, h), int(c[0]["bounce_count"]))
        want.setflags(write=False)
        _LENS_WANT[key] = (c, lens, want, n_rays)
    return _LENS_WANT[key]


@pytest.mark.parametrize("lens_rule", ["thin", "ortho"])
def test_lens_views_of_the_randomized_scenes_hit_something(oracle, lens_rule):
    """At least 20 of the 40 views per rule cast more rays than paths at the scene's own bounce count (which is then at least 1)."""
    hit = []
    for i, case in enumerate(sc.random_scenes()):
        c, _, want, n_rays = _lens_want(oracle, "random", i, "own", lens_rule)
        if int(c[0]["bounce_count"]) >= 1 and n_rays > case[4] * case[5]:
            hit.append(i)
    print(f"{lens_rule} views of the randomized scenes that cast more rays than paths: {len(hit)} of {sc.N_SCENES}: {hit}")
    assert len(hit) >= MIN_LENS_VIEWS, hit


@pytest.mark.parametrize("lens_rule", ["thin", "ortho"])
def test_lens_views_of_the_boards_meet_their_spheres(oracle, lens_rule):
    """The lane board holds under a board's lens views: the twin's ray of pixel k meets the sphere of material k in every pixel (all
    eight boards have their 64 spheres), in both trees, and the view casts more rays than paths."""
    for name in LENS_BOARDS:
        for tree in ("ploc", "median3"):
            b, _, cam, win, w, h = _board(name, tree)
            c, lens, want, n_rays = _lens_want(oracle, "board", name, tree, lens_rule)
            rays = _twin_rays(c, win, lens, w, h)
            hit = qr.expected(oracle, b.models, b.bvh, qr.make_rays(rays["origin"], rays["direction"]))[0]["material"]
            assert hit.tolist() == list(range(w * h)), (name, tree, hit.tolist())
            assert n_rays > w * h, (name, tree, n_rays)


# ---- GPU: what every launch is held to -----------------------------------------------------------------------------------------------------

_TABLE = {}        # (rule, form, placement, flavour) -> launches whose `rays` was greater than 0
_DONE = set()      # the GPU cases that have run in this process


def _ran(rule, st, tree_flavour):
    stream = st["kernel_variant"] in (PIXELS_STREAM, LENS_STREAM)
    key = (rule, "stream", PLACEMENT[st["scene_in_lds"]], tree_flavour) if stream else (rule, "plain", "-", tree_flavour)
    _TABLE[key] = _TABLE.get(key, 0) + (1 if st["rays"] > 0 else 0)


def _assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[:4].tolist()}"


def _list_call(plugin, cam, win, w, h, lst, run, lens=None):
    """The list through one run -- a residency of the streaming form or the plain form on the device entry point, or the host entry
    point -- -> ((n, 4) f32, stats, expected kernel_variant, expected scene_in_lds).  The bytes behind the last entry keep their fill."""
    import torch
    stream_variant, plain_variant = (LENS_STREAM, LENS_PLAIN) if lens is not None else (PIXELS_STREAM, PIXELS_PLAIN)
    if run == "host":
        got = plugin.node.render_pixels(cam, win, w, h, lst) if lens is None else plugin.node.render_lens_pixels(cam, win, lens, w, h, lst)
        return got, dict(plugin.node.last_stats), stream_variant, 1
    knobs, in_lds = RESIDENCIES.get(run, ({}, 0))
    flags = brt.FLAG_KERNEL_SIMPLE if run == "plain" else 0
    d_px = dev(lst)
    out = guarded(lst.size * 16, GUARD, FILL)
    with plugin.tuning(**knobs):
        if lens is None:
            plugin.node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), lst.size, out.data_ptr(), flags=flags)
        else:
            plugin.node.render_lens_pixels_device(cam, win, lens, w, h, d_px.data_ptr(), lst.size, out.data_ptr(), flags=flags)
    st = dict(plugin.node.last_stats)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[lst.size * 16:] == FILL).all(), "the guard behind the last entry was written"
    return raw[:lst.size * 16].view(F32).reshape(-1, 4).copy(), st, (plain_variant if run == "plain" else stream_variant), in_lds


def _check_list(got, st, variant, in_lds, lst, want, pixel_rays, spp, what):
    """The asserts of a list: traced entries, refused entries, rays, paths, reserved, the form and the residency that ran."""
    ok = lst < want.shape[0]
    assert st["kernel_variant"] == variant, (what, st["kernel_variant"])
    assert st["scene_in_lds"] == in_lds, (what, st["scene_in_lds"])
    assert not got[~ok].view(np.uint32).any(), f"{what}: a refused entry is not four zeros"
    _assert_bits(got[ok], want[lst[ok]], what)
    if pixel_rays is not None:
        assert st["rays"] == int(pixel_rays[lst[ok]].sum(dtype=np.int64)), (what, st["rays"])
    assert st["paths"] == int(ok.sum()) * spp, (what, st["paths"])
    assert st["reserved"] == int((~ok).sum()), (what, st["reserved"])
    assert st["tree_rebuilt"] == 0, what


def test_the_checker_sees_every_kind_of_difference():
    """_check_list on made-up values: it passes the values themselves and a NaN of another payload, and fails on a flipped bit, a number
    for a NaN, a NaN for a number, a written refused entry, and every count or stat that is off by one."""
    w, h, spp = 5, 7, 3
    rng = np.random.default_rng(11)
    lst = scene_list(w, h, 5)
    want = rng.random((w * h, 4), dtype=F32)
    want[3, 1] = np.nan
    pixel_rays = rng.integers(1, 9, w * h).astype(np.uint32)
    ok = lst < w * h
    good = np.zeros((lst.size, 4), F32)
    good[ok] = want[lst[ok]]
    st = {"kernel_variant": PIXELS_STREAM, "scene_in_lds": 2, "rays": int(pixel_rays[lst[ok]].sum()), "paths": int(ok.sum()) * spp,
          "reserved": int((~ok).sum()), "tree_rebuilt": 0}
    check = lambda got, stats: _check_list(got, stats, PIXELS_STREAM, 2, lst, want, pixel_rays, spp, "made up")
    check(good, st)
    at_nan, at_bad, at_ok = int(np.flatnonzero(lst == 3)[0]), int(np.flatnonzero(~ok)[0]), int(np.flatnonzero(ok)[0])
    other_nan = good.copy()
    other_nan.view(np.uint32)[at_nan, 1] = 0xFFC12345
    check(other_nan, st)
    edits = {"bit": lambda g: g.view(np.uint32).__setitem__((at_ok, 2), g.view(np.uint32)[at_ok, 2] ^ 1),
             "number for NaN": lambda g: g.__setitem__((at_nan, 1), 0.5), "NaN for number": lambda g: g.__setitem__((at_ok, 0), np.nan),
             "refused written": lambda g: g.__setitem__((at_bad, 3), 1.0)}
    for name, edit in edits.items():
        bad = good.copy()
        edit(bad)
        with pytest.raises(AssertionError):
            check(bad, st)
    for field in st:
        with pytest.raises(AssertionError):
            check(good, {**st, field: st[field] + 1})


# ---- GPU: pinhole lists on the randomized and wild scenes ----------------------------------------------------------------------------------

_WANT = {}
SCENE_RUNS = ("lds", "lds_top", "global", "plain", "host")


def _pure(lvl):
    out = lvl.copy()
    out["level"] = int(brt.Raytracing.Pure)
    return out


def _want_scene(oracle, kind, i):
    """(the oracle's Pure frame without raster inputs as (n, 4), the rays every pixel casts) of scene i of a table, once; None where
    the library refuses the scene."""
    key = (kind, i)
    if key not in _WANT:
        b, lvl, cam, win, w, h = _SCENES[kind]()[i][:6]
        try:
            brt.validate_scene(b.models, b.materials, b.bvh)
        except brt.BrtError:
            _WANT[key] = None
        else:
            frame, cnt = oracle.render(b, _pure(lvl), cam, win, w, h)
            rays = oracle.pixel_rays(b, cam, win, w, h).reshape(-1)
            assert int(rays.sum(dtype=np.int64)) == cnt["rays"]
            frame = np.asarray(frame, F32).reshape(-1, 4)
            frame.setflags(write=False)
            _WANT[key] = (frame, rays)
    return _WANT[key]


def _scenes_run(plugin, oracle, kind, run):
    if ("scenes", kind, run) in _DONE:
        return
    for i, (b, lvl, cam, win, w, h, _, _) in enumerate(_SCENES[kind]()):
        spp = int(cam[0]["sample_count"])
        what = f"{kind} case {i}: {len(b.models)} spheres, {len(b.bvh)} nodes, {w}x{h}, {spp} spp, {int(cam[0]['bounce_count'])} bounces, {run}"
        want = _want_scene(oracle, kind, i)
        lst = scene_list(w, h, [i, len(kind)])
        if want is None:
            with pytest.raises(brt.BrtError):
                plugin.node.write_buffers(b)
                _list_call(plugin, cam, win, w, h, lst, run)
            continue
        plugin.node.write_buffers(b)
        got, st, variant, in_lds = _list_call(plugin, cam, win, w, h, lst, run)
        _check_list(got, st, variant, in_lds, lst, want[0], want[1], spp, what)
        if spp == 0:
            assert st["rays"] == 0, what
        _ran("pinhole", st, _flavour_of((kind, i), b))
    _DONE.add(("scenes", kind, run))


@pytest.mark.gpu
@pytest.mark.parametrize("run", SCENE_RUNS)
@pytest.mark.parametrize("kind", list(_SCENES))
def test_pinhole_lists_on_randomized_and_wild_scenes(plugin, oracle, kind, run):
    """40 randomized scenes (fractional metallic and transmission, ior below 1, chains, multi-sphere leaves) and 40 wild ones (special
    radii, positions and material fields, coincident spheres, poisoned boxes, window height 0, special seeds, 0 and 64 samples, 70
    bounces): every entry is its pixel of the oracle's Pure frame, refused entries are zeros, the counts are the oracle's."""
    _scenes_run(plugin, oracle, kind, run)


# ---- GPU: the boards, the lane pattern chosen through the list -----------------------------------------------------------------------------

BOARD_RUNS = ("lds", "lds_top", "global", "plain")


def _want_board(oracle, name, tree):
    key = ("board", name, tree)
    if key not in _WANT:
        b, lvl, cam, win, w, h = _board(name, tree)
        frame, cnt = oracle.render(b, lvl, cam, win, w, h)
        rays = oracle.pixel_rays(b, cam, win, w, h).reshape(-1)
        assert int(rays.sum(dtype=np.int64)) == cnt["rays"]
        frame = np.asarray(frame, F32).reshape(-1, 4)
        frame.setflags(write=False)
        _WANT[key] = (frame, rays)
    return _WANT[key]


def _board_run(plugin, oracle, name, tree):
    if ("board", name, tree) in _DONE:
        return
    b, lvl, cam, win, w, h = _board(name, tree)
    want, pixel_rays = _want_board(oracle, name, tree)
    plugin.node.write_buffers(b)
    for which, lst in board_lists(w, h, [len(name), w, h]).items():
        for run in BOARD_RUNS:
            got, st, variant, in_lds = _list_call(plugin, cam, win, w, h, lst, run)
            _check_list(got, st, variant, in_lds, lst, want, pixel_rays, sc.SPP, f"{name} under {tree}, list ({which}), {run}")
            _ran("pinhole", st, _flavour_of(("board", name, tree), b))
    _DONE.add(("board", name, tree))


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("name", list(sc.PURE))
def test_boards_with_the_lane_pattern_chosen_through_the_list(plugin, oracle, name, tree):
    """Patterns at 1 and 6 bounces, ladders, lottery, glass, colours and the small boards; per tree the lists (a), (b), (c) under three
    residencies of the streaming form and in the plain form.  An enclosed board's frame is 0 or NaN everywhere: there `rays` is the
    witness (paths that run to the bounce limit beside absorbed ones, refilled out of step in list (c))."""
    _board_run(plugin, oracle, name, tree)


# ---- GPU: the two lens rules ---------------------------------------------------------------------------------------------------------------

LENS_RUNS = ("lds", "lds_top", "global", "plain", "list")


def _lens_frame_dev(plugin, cam, win, lens, w, h):
    import torch
    buf = guarded(w * h * 16, GUARD, FILL)
    plugin.node.render_lens_device(cam, win, lens, w, h, buf.data_ptr())
    st = dict(plugin.node.last_stats)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[w * h * 16:] == FILL).all(), "the guard behind the frame was written"
    return raw[:w * h * 16].view(F32).reshape(-1, 4).copy(), st


def _lens_run(plugin, oracle, kind, which, tree, run):
    if ("lens", kind, which, tree, run) in _DONE:
        return
    b, _, cam, win, w, h = _lens_scene(kind, which, tree)
    tree_flavour = _flavour_of((kind, which) if kind == "random" else (kind, which, tree), b)
    plugin.node.write_buffers(b)
    for lens_rule in ("thin", "ortho"):
        c, lens, want, n_rays = _lens_want(oracle, kind, which, tree, lens_rule)
        what = f"{kind} {which} ({tree} tree, {len(b.models)} spheres, {w}x{h}, {int(c[0]['bounce_count'])} bounces), {lens_rule}, {run}"
        if run == "list":
            lst = scene_list(w, h, [w, h, 77], repeats=False)
            got, st, variant, in_lds = _list_call(plugin, c, win, w, h, lst, "lds", lens)
            _check_list(got, st, variant, in_lds, lst, want, None, 1, what)
        else:
            if run == "plain":
                got, variant, in_lds = plugin.node.render_lens(c, win, lens, w, h, brt.FLAG_KERNEL_SIMPLE).reshape(-1, 4), LENS_PLAIN, 0
                st = dict(plugin.node.last_stats)
            else:
                knobs, in_lds = RESIDENCIES[run]
                with plugin.tuning(**knobs):
                    got, st = _lens_frame_dev(plugin, c, win, lens, w, h)
                variant = LENS_STREAM
            assert (st["kernel_variant"], st["scene_in_lds"]) == (variant, in_lds), (what, st)
            assert (st["paths"], st["reserved"], st["tree_rebuilt"]) == (w * h, 0, 0), (what, st)
            _assert_bits(got, want, what)
        assert st["rays"] == n_rays, (what, st["rays"], n_rays)
        _ran(lens_rule, st, tree_flavour)
    _DONE.add(("lens", kind, which, tree, run))


@pytest.mark.gpu
@pytest.mark.parametrize("run", LENS_RUNS)
@pytest.mark.parametrize("kind", ["random", "board"])
def test_lens_rules_at_one_sample(plugin, oracle, kind, run):
    """Thin lens and orthographic view of all 40 randomized scenes and of eight boards in two trees, as
    test_lens.py::test_thin_lens_and_orthographic_frames_at_one_sample states them: the streaming form under three residencies on
    render_lens_device, the plain form through render_lens, a shuffled list with refused entries through render_lens_pixels_device."""
    for case in LENS_CASES:
        if case[0] == kind:
            _lens_run(plugin, oracle, *case, run)


# Several samples: two GENERAL trees of the randomized table, a single leaf (11 spheres, 5 bounces) and a median split with multi-sphere
# leaves (15 spheres under 13 nodes, 2 bounces).  At most 96 pixels per combination, the size test_lens.py pays for.
SEVERAL = {"single_leaf": 37, "median_split": 0}
SEVERAL_PIXELS = 96


def _several_view(i, mode, spp):
    b, _, cam, win, w, h = sc.random_scenes()[i][:6]
    c, lens = (cam.copy(), brt.lens(0.0)) if mode == "pinhole" else _lens_view("random", cam, mode)
    c["sample_count"] = spp
    return b, c, win, lens, w, h


@functools.lru_cache(maxsize=None)
def _several_want(i, mode, spp):
    b, c, win, lens, w, h = _several_view(i, mode, spp)
    pixels = np.random.default_rng([i, 13]).permutation(w * h)[:SEVERAL_PIXELS].astype(np.uint32)
    sh = npr.Shader(b.models, b.materials, b.bvh, c[0], win[0], 3)
    want = np.array([lr.pixel(sh, c, win, lens, w, h, int(p) % w, int(p) // w) for p in pixels])
    return pixels, want


def test_the_several_sample_scenes_are_general_trees():
    single, median = (sc.random_scenes()[SEVERAL[k]][0] for k in ("single_leaf", "median_split"))
    assert len(single.bvh) == 1 and single.bvh[0]["model_count"] == len(single.models) > 1
    assert len(median.bvh) > 1 and (median.bvh["model_count"][sorted(_reachable(median.bvh))] > 1).any()
    assert _flavour_of(("random", SEVERAL["single_leaf"]), single) == _flavour_of(("random", SEVERAL["median_split"]), median) == "general"
    # the three rules say different things about these scenes: at 2 samples each lens rule changes at least half of the listed pixels
    # against the pinhole's, and no rule's list is one value
    for tree, i in SEVERAL.items():
        pin, thin, ortho = (_several_want(i, mode, 2)[1].view(np.uint32) for mode in ("pinhole", "thin", "ortho"))
        changed = [float((other != pin).any(axis=1).mean()) for other in (thin, ortho)]
        distinct = [len({tuple(p) for p in v.tolist()}) for v in (pin, thin, ortho)]
        print(f"{tree} scene {i}: thin / ortho change {changed} of the pixels, distinct values {distinct}")
        assert min(changed) >= 0.5 and min(distinct) >= 8, (tree, changed, distinct)


def _several_run(plugin, tree, spp):
    if ("several", tree, spp) in _DONE:
        return
    i = SEVERAL[tree]
    plugin.node.write_buffers(sc.random_scenes()[i][0])
    for mode in ("pinhole", "thin", "ortho"):
        b, c, win, lens, w, h = _several_view(i, mode, spp)
        pixels, want = _several_want(i, mode, spp)
        for run in ("lds", "plain"):
            got, st, variant, in_lds = _list_call(plugin, c, win, w, h, pixels, run, None if mode == "pinhole" else lens)
            _check_list(got, st, variant, in_lds, pixels, _scatter(want, pixels, w * h), None, spp, f"{tree} scene {i}, {mode}, {spp} spp, {run}")
            _ran(mode, st, _flavour_of(("random", i), b))
    _DONE.add(("several", tree, spp))


def _scatter(values, pixels, n):
    frame = np.zeros((n, 4), F32)
    frame[pixels] = values
    return frame


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [2, 5])
@pytest.mark.parametrize("tree", list(SEVERAL))
def test_several_samples_against_the_restatement(plugin, tree, spp):
    """The samples of a pixel chain one RNG state through the lens rule and the shader, which only the numpy restatement states
    (lens_ref.pixel on npr.Shader): a shuffled list of at most 96 pixels at 2 and 5 samples under the pinhole (brt_render_pixels_device),
    the thin lens and the orthographic camera (brt_render_lens_pixels_device), both forms."""
    _several_run(plugin, tree, spp)


# ---- the table of instantiations that ran --------------------------------------------------------------------------------------------------

RULES = ("pinhole", "thin", "ortho")
CELLS = [(rule, "stream", placement, tree) for rule in RULES for placement in ("LDS", "LDS_TOP", "GLOBAL") for tree in ("simple", "general")] + [
    (rule, "plain", "-", tree) for rule in RULES for tree in ("simple", "general")]


@pytest.mark.gpu
def test_every_instantiation_ran(plugin, oracle):
    """Every cell of {pinhole, thin, ortho} x {LDS, LDS_TOP, GLOBAL} x {simple, general} of k_list_stream with 16-bit descriptors, and of
    k_list_plain per rule x {simple, general}, holds at least 10 launches that cast rays.  (The tests above fill the table; what has not
    run yet -- this test selected alone -- runs here.)  Left out: k_list_stream<*, SCENE_GLOBAL, false, false>, the global-memory cell
    of 32-bit descriptors under a general tree, which needs more than 16 382 spheres under a hand-made tree (minutes on the oracle)."""
    for kind in _SCENES:
        for run in SCENE_RUNS:
            _scenes_run(plugin, oracle, kind, run)
    for name in sc.PURE:
        for tree in TREES:
            _board_run(plugin, oracle, name, tree)
    for run in LENS_RUNS:
        for case in LENS_CASES:
            _lens_run(plugin, oracle, *case, run)
    for tree in SEVERAL:
        for spp in (2, 5):
            _several_run(plugin, tree, spp)
    print("rule     form    placement  tree     launches with rays > 0")
    for key in CELLS:
        print(f"{key[0]:8s} {key[1]:7s} {key[2]:10s} {key[3]:8s} {_TABLE.get(key, 0)}")
    assert set(_TABLE) <= set(CELLS), set(_TABLE) - set(CELLS)
    short = {key: _TABLE.get(key, 0) for key in CELLS if _TABLE.get(key, 0) < MIN_LAUNCHES}
    assert not short, short
