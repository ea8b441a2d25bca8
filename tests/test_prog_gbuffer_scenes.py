"""The progressive rule of the list tracers (ProgStart in k_list_plain / k_list_stream, brt_progressive.hip and brt_pixels_dev.h) and the
G-buffer kernel (k_gbuffer, brt_gbuffer.hip) on general trees and hostile scenes: the 40 randomized and 40 wild scenes and the lane
boards of tests/shade_cases.py, each under its own tree and under a median-split tree of three-sphere leaves (the boards also under one
leaf of every sphere), bit for bit against the C oracle.  (tests/test_progressive.py, tests/test_pixel_rules.py and tests/test_gbuffer.py
render simple trees only.)

  * CPU: the case tables are what they claim, on the oracle alone -- the centre rays of the scenes hit and miss, the 3-sample frames cast
    more rays than paths and (wild table) hold NaN / INF colours, every median-split tree is a GENERAL one, the wild table clears
    boxes_ordered and spheres_bounded, every wave of a mixed-record board holds all three record kinds, the one-call thresholds select
    some pixels and not all on a model of the records, the deep tree's overflow rule fires.
  * GPU, progressive: the scenes to 1 and on to 3 samples under three residencies of the streaming form and in the plain form, the list
    shape rotating (null list in tile order, in raster order, a shuffled list with refused entries), the host entry point; the boards
    with the lane pattern chosen through the list; boards whose records start finished, empty and half-way; the moments sample by sample
    under NaN / INF colours; a 16 383-sphere scene under three-sphere leaves (32-bit descriptors); the one-call form on general trees;
    the table of instantiations that ran.
  * GPU, G-buffer: the hit planes of every scene and of the boards under one 64-sphere leaf against oracle_raycast on the tree the GPU
    walked, the sphere id through query_ref.check_spheres; the derived planes, coverage, a tree deeper than the stack, 32-bit descriptors
    with three-sphere leaves.

Every comparison is an equality of bits; a NaN equals a NaN at the same place whatever its sign and payload (which NaN an operation
returns is the machine's choice), in sum, m1, m2, the frames and the f32 planes: both sides pass through test_gbuffer._canon before the
checkers of the features' own test files (test_progressive._check_step, test_gbuffer._assert_planes) compare them.  rng, n, rays, ids
and the packed formats compare exactly.

Measured where this file was written (one MI355X, 16 granted CPUs): the 18 CPU tests 4.7 s (the host twin's rays 2.6 s, the oracle's
centre hits and 3-sample frames the rest), the 195 GPU tests 12.2 s including their share of the oracle; the slowest GPU case 1.4 s
(16 383 spheres under three-sphere leaves: the oracle's two frames and pixel_rays), no other above 1 s.

Two deliberate one-line breaks, each tried on a scratch copy of the library: k_gbuffer reading sv.sphere_material at the leaf's first
sphere fails 17 tests here (every G-buffer scene table, the single-leaf boards, the derived planes, coverage, the 32-bit case) while
tests/test_gbuffer.py stays green; ProgStart::begin without `lane.m1 = 0.0f` fails test_progressive_refills_on_a_general_tree here and
tests/test_progressive.py::test_a_list_longer_than_the_launch_has_lanes, and nothing else: below the launch's lane cap no lane ever
takes a second pixel (see the note above that test)."""
import numpy as np
import pytest

import bevyray_amd as brt
import gbuffer_cases as gc
import gbuffer_ref as gr
import progressive_ref as pr
import query_ref as qr
import shade_cases as sc
from helpers import BIG_VIEW, big_scene, big_view, chain_bvh, cover, graft_bvh, median_split_bvh
from test_gbuffer import DESCS, PLANES, _assert_planes, _canon, _device, _expected_planes, _hits_of_rays, _twin_planes
from test_gbuffer import FILL as COV_FILL
from test_list_tracers_scenes import (LENS_BOARDS, MIN_LAUNCHES, MIN_PER_FLAVOUR, PLACEMENT, RESIDENCIES, TREES, _board, _pure, _with_refused,
                                      board_lists, boxes_ordered, flavour, spheres_bounded)
from test_progressive import FORMS, REC, Planes, View, _bytes, _check_step

F32 = np.float32
STREAM_FORM, PLAIN_FORM = FORMS[0][1], FORMS[1][1]          # brt_stats::kernel_variant: 36, 37
TARGETS = (1, 3)
SCENE_TREES = ("ploc", "median3")                            # "ploc": the scene's own tree, as test_list_tracers_scenes names it
RUNS = ("lds", "lds_top", "global", "plain")
MAX_REFUSED = 4                                              # views of a table the entry point may refuse by a documented rule
_SCENES = {"random": sc.random_scenes, "wild": sc.wild_scenes}
# the bars of the case tables (measured on the oracle: 34 of the randomized, 14 and 29 of the wild scenes; 34 and 26; 10)
MIN_HIT_AND_MISS = {"random": 30, "wild": 12}
MIN_WILD_WITH_A_HIT = 28
MIN_MORE_RAYS_THAN_PATHS = {"random": 30, "wild": 22}
MIN_WILD_NON_FINITE = 8


# ---- NaN-blind bytes --------------------------------------------------------------------------------------------------------------------

def _canon_f32(a):
    """An f32 array with every NaN the same NaN."""
    return _canon(a).view(F32).reshape(np.shape(a))


def _canon_state(state):
    out = state.copy()
    for k in ("sum", "m1", "m2"):
        out[k] = _canon_f32(out[k])
    return out


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


class CanonPlanes(Planes):
    """test_progressive.Planes (RGBA32F) read back with every NaN the same NaN."""

    def state(self):
        return _canon_state(super().state())

    def frame(self):
        raw = super().frame()
        return _canon(raw.view(F32)).view(np.uint8).reshape(raw.shape)


class CanonView(View):
    """test_progressive.View with every NaN of the oracle's frames the same NaN."""

    def __init__(self, oracle, buffers, view_of, w, h):
        super().__init__(oracle, buffers, view_of, w, h)
        self._want = {}

    def want(self, n):
        if n not in self._want:
            lvl, cam, _ = self.view_of(n)
            frame, cnt = self.oracle.render(self.b, lvl, cam, self.win, self.w, self.h)
            rays = self.oracle.pixel_rays(self.b, cam, self.win, self.w, self.h)
            assert int(rays.sum(dtype=np.int64)) == cnt["rays"]
            frame = _canon_f32(frame)
            frame.setflags(write=False)
            rays.setflags(write=False)
            self._want[n] = (frame, rays)
        return self._want[n]

    def rays_to(self, n):
        return 0 if n == 0 else int(self.want(n)[1].sum(dtype=np.int64))


# ---- the scenes, their trees and what the oracle says of them, once ---------------------------------------------------------------------------

_VIEWS, _FLAVOUR, _HITS = {}, {}, {}


def _scene(kind, i, tree):
    b, lvl, cam, win, w, h = _SCENES[kind]()[i][:6]
    return TREES[tree](b), lvl, cam, win, w, h


def _flavour_of(key, b):
    if key not in _FLAVOUR:
        _FLAVOUR[key] = flavour(b)
    return _FLAVOUR[key]


def _view_at(lvl, cam, win):
    def view_of(n):
        c = cam.copy()
        c["sample_count"] = n
        return _pure(lvl), c, win
    return view_of


def _scene_view(oracle, kind, i, tree):
    """The scene under `tree` with its own camera, window and bounce count, the level forced to Pure, the sample count the target's."""
    key = (kind, i, tree)
    if key not in _VIEWS:
        b, lvl, cam, win, w, h = _scene(kind, i, tree)
        _VIEWS[key] = CanonView(oracle, b, _view_at(lvl, cam, win), w, h)
    return _VIEWS[key]


def _board_view(oracle, name, tree):
    key = ("board", name, tree)
    if key not in _VIEWS:
        b, lvl, cam, win, w, h = _board(name, tree)
        _VIEWS[key] = CanonView(oracle, b, _view_at(lvl, cam, win), w, h)
    return _VIEWS[key]


def _pixel_rays(oracle, cam, win, w, h):
    """query_ref.pixel_rays with the term its vectorised arithmetic leaves out: camera_ray_dir_center adds (1 / window size) * 0 to the
    pixel's position, as query_ref.pixel_ray_np restates it, and under a window of height 0 (the wild table has two) that is INF * 0:
    every ray of the view is NaN and misses.  For a finite window size the term is +0.0 and changes no bit.  (Held against the
    compiled twin brt.pixel_ray in test_the_centre_rays_are_the_host_twins.)"""
    rays = qr.pixel_rays(oracle, cam, w, h)
    with np.errstate(all="ignore"):
        height = F32(win[0]["height"])
        terms = (F32(1.0) / (height * F32(cam[0]["aspect"]))) * F32(0.0), (F32(1.0) / height) * F32(0.0)
    if not np.isfinite(terms).all():
        rays["direction"] = np.nan
    return rays


def _centre_hits(oracle, key, b, cam, win, w, h):
    """(rays, the oracle's records, hit mask) of the pixel-centre rays of a view on b's tree, once per key."""
    if key not in _HITS:
        rays = _pixel_rays(oracle, cam, win, w, h)
        want, _ = qr.expected(oracle, b.models, b.bvh, rays)
        _HITS[key] = (rays, want, (want["status"] & brt.QUERY_STATUS_HIT) != 0)
    return _HITS[key]


def _scene_hits(oracle, kind, i, tree):
    b, _, cam, win, w, h = _scene(kind, i, tree)
    return _centre_hits(oracle, (kind, i, tree), b, cam, win, w, h)


# ---- the lists --------------------------------------------------------------------------------------------------------------------------

LIST_SHAPES = ("tile", "raster", "shuffled")


def _list_of(shape, w, h, seed):
    """-> (host list or None, knobs): a null list in tile order, a null list in raster order, or every pixel exactly once in a shuffled
    order with refused entries at places 0, 31, 32, 63 and 64."""
    if shape == "tile":
        return None, {"BRT_PROGRESSIVE_ORDER": 1}
    if shape == "raster":
        return None, {"BRT_PROGRESSIVE_ORDER": 0}
    lst = _with_refused(np.random.default_rng(seed).permutation(w * h).astype(np.int64), w * h)
    return lst, {}


def _no_repeats(lst, n_px):
    ok = lst[lst < n_px]
    return np.unique(ok).size == ok.size


def test_the_lists_name_every_pixel_at_most_once():
    """The contract allows a pixel at most once per call: the shuffled lists name every pixel exactly once, the board lists (a) and (b)
    every pixel once with refused entries between."""
    for w, h in ((1, 1), (5, 7), (8, 8), (69, 47), (89, 172)):
        lst, _ = _list_of("shuffled", w, h, [w, h])
        ok = lst < w * h
        assert np.array_equal(np.sort(lst[ok]), np.arange(w * h)) and _no_repeats(lst, w * h)
        assert (~ok).sum() == sum(1 for j, p in enumerate((0, 31, 32, 63, 64)) if p <= w * h + j), (w, h)
    for w, h in sc.SMALL_SIZES:
        ls = board_lists(w, h, 3)
        for which in ("a", "b"):
            assert _no_repeats(ls[which], w * h) and (ls[which] < w * h).sum() == w * h
        assert not _no_repeats(ls["c"], w * h) or w * h == 0          # (list "c" repeats pixels: it is not used here)


# ---- CPU: the case tables are what they claim ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(_SCENES))
def test_the_centre_rays_are_the_host_twins(oracle, kind):
    """The rays the oracle walks are the rays brt_host_pixel_ray (the code the kernels compile) gives: the corners and 60 random pixels
    of every view, bit for bit, a NaN for a NaN."""
    rng = np.random.default_rng(5)
    nan_views = []
    for i, (b, lvl, cam, win, w, h, _, _) in enumerate(_SCENES[kind]()):
        rays = _scene_hits(oracle, kind, i, "ploc")[0]
        if np.isnan(rays["direction"]).all():
            nan_views.append(i)
        for p in np.unique(np.concatenate([[0, w - 1, w * h - w, w * h - 1], rng.integers(0, w * h, 60)])):
            twin = brt.pixel_ray(cam, win, w, h, int(p % w), int(p // w))[0]
            assert np.array_equal(_canon(twin["direction"]), _canon(rays[p]["direction"])), (kind, i, int(p))
            assert np.array_equal(_canon(twin["origin"]), _canon(rays[p]["origin"])), (kind, i, int(p))
    print(f"{kind} views whose every centre ray is NaN: {nan_views}")


@pytest.mark.parametrize("kind", list(_SCENES))
def test_centre_rays_hit_and_miss(oracle, kind):
    """The G-buffer's rays on the scenes' own trees: most views see both a sphere and the sky."""
    both, any_hit = [], []
    for i in range(sc.N_SCENES):
        hit = _scene_hits(oracle, kind, i, "ploc")[2]
        if hit.any():
            any_hit.append(i)
            if not hit.all():
                both.append(i)
    print(f"{kind} scenes whose centre rays hit and miss: {len(both)} {both}; with at least one hit: {len(any_hit)}")
    assert len(both) >= MIN_HIT_AND_MISS[kind], both
    if kind == "wild":
        assert len(any_hit) >= MIN_WILD_WITH_A_HIT, any_hit


@pytest.mark.parametrize("kind", list(_SCENES))
def test_three_sample_frames_bounce_and_hold_special_values(oracle, kind):
    """At 3 samples and the scene's own bounce count most views cast more rays than paths; in the wild table the frames of at least 8
    scenes hold a NaN or an INF: the progressive sums and moments meet such colours."""
    more, special = [], []
    for i, case in enumerate(_SCENES[kind]()):
        view = _scene_view(oracle, kind, i, "ploc")
        frame, rays = view.want(3)
        if int(rays.sum(dtype=np.int64)) > 3 * view.w * view.h:
            more.append(i)
        if not np.isfinite(frame).all():
            special.append(i)
    print(f"{kind} scenes that cast more rays than paths at 3 spp: {len(more)} {more}; with a non-finite value in the frame: {len(special)} {special}")
    assert len(more) >= MIN_MORE_RAYS_THAN_PATHS[kind], more
    if kind == "wild":
        assert len(special) >= MIN_WILD_NON_FINITE, special


@pytest.mark.parametrize("kind", list(_SCENES))
def test_trees_of_both_flavours(kind):
    """Each scene is used under its own tree and under the median split of three-sphere leaves, which is a GENERAL tree wherever the
    scene has two spheres; over both trees each table holds at least 15 simple and 15 general ones, and the library refuses none."""
    tally = {"simple": 0, "general": 0}
    for i, case in enumerate(_SCENES[kind]()):
        for tree in SCENE_TREES:
            f = _flavour_of((kind, i, tree), _scene(kind, i, tree)[0])
            tally[f] += 1
            if tree == "median3" and len(case[0].models) >= 2:
                assert f == "general", (kind, i)
    print(f"{kind} scenes under their own and the median-split tree: {tally['simple']} simple, {tally['general']} general trees")
    assert tally["simple"] >= MIN_PER_FLAVOUR and tally["general"] >= MIN_PER_FLAVOUR, tally


def test_wild_scenes_clear_the_walk_flags_under_both_trees():
    """Spheres that fail spheres_bounded and child boxes that fail boxes_ordered (a median split over a NaN centre has such boxes too)
    reach both kernels: at least one scene of each kind per tree, among those whose centre rays are walked at all."""
    for tree in SCENE_TREES:
        unordered = [i for i in range(sc.N_SCENES) if not boxes_ordered(_scene("wild", i, tree)[0].bvh)]
        unbounded = [i for i in range(sc.N_SCENES) if not spheres_bounded(_scene("wild", i, tree)[0].models)]
        print(f"wild scenes under {tree} that clear boxes_ordered: {unordered}; spheres_bounded: {unbounded}")
        assert len(unordered) >= 1 and len(unbounded) >= 1


# ---- GPU: what every progressive launch is held to ---------------------------------------------------------------------------------------

_TABLE = {}        # (form, placement, flavour, descriptor width) -> launches whose `rays` was greater than 0
_DONE = set()      # the GPU cases that have run in this process
_REFUSED = {}      # (family, kind) -> the scenes whose view the entry point refused


def _ran(st, tree_flavour, width=16):
    key = ("stream", PLACEMENT[st["scene_in_lds"]], tree_flavour, width) if st["kernel_variant"] == STREAM_FORM else ("plain", "-", tree_flavour, width)
    _TABLE[key] = _TABLE.get(key, 0) + (1 if st["rays"] > 0 else 0)


def _step(plugin, oracle, view, planes, n_from, n_to, run, shape, seed, what, tree_flavour, width=16, in_lds=None):
    """One call that takes every pixel of `planes` from n_from to n_to samples through `run` (a residency of the streaming form, or the
    plain form) with a list of `shape`; then n, rays, the frame bytes (test_progressive._check_step) and the stats."""
    from helpers import dev
    knobs, want_lds = RESIDENCIES.get(run, ({}, None))
    if in_lds is not None:
        want_lds = in_lds
    flags, variant = FORMS[1] if run == "plain" else FORMS[0]
    lst, order = (shape, {}) if isinstance(shape, np.ndarray) else _list_of(shape, view.w, view.h, seed)
    n_px = view.w * view.h
    with plugin.tuning(**knobs, **order):
        if lst is None:
            st = planes.sample(plugin, view.cam, view.win, n_to, flags=flags)
            refused = 0
        else:
            assert _no_repeats(lst, n_px)
            d_list = dev(lst)
            st = planes.sample(plugin, view.cam, view.win, n_to, d_list.data_ptr(), lst.size, flags=flags)
            refused = int((lst >= n_px).sum())
    assert st["kernel_variant"] == variant, (what, st["kernel_variant"])
    if variant == STREAM_FORM and want_lds is not None:
        assert st["scene_in_lds"] == want_lds, (what, st["scene_in_lds"])
    _check_step(oracle, view, planes, n_to, what)
    assert st["rays"] == view.rays_to(n_to) - view.rays_to(n_from), (what, st["rays"])
    assert st["paths"] == n_px * (n_to - n_from), (what, st["paths"])
    assert st["reserved"] == refused, (what, st["reserved"])
    assert st["tree_rebuilt"] == 0, what
    _ran(st, tree_flavour, width)
    return st


def _refusal(family, kind, i, error):
    """A view the entry point refuses by a documented rule: an invalid argument or an unsupported one, with its text."""
    assert error.code in (-1, -8) and error.text, (family, kind, i, error)
    _REFUSED.setdefault((family, kind), set()).add(i)
    assert len(_REFUSED[family, kind]) <= MAX_REFUSED, (family, kind, sorted(_REFUSED[family, kind]))


# ---- GPU 2(a): the scenes ------------------------------------------------------------------------------------------------------------------

def _prog_scenes_run(plugin, oracle, kind, tree):
    if ("prog scenes", kind, tree) in _DONE:
        return
    for i in range(sc.N_SCENES):
        view = _scene_view(oracle, kind, i, tree)
        b, w, h = view.b, view.w, view.h
        fl = _flavour_of((kind, i, tree), b)
        plugin.node.write_buffers(b)
        try:
            CanonPlanes(w, h).sample(plugin, view.cam, view.win, 1)
        except brt.BrtError as e:
            _refusal("progressive", kind, i, e)
            continue
        for r, run in enumerate(RUNS):
            shape = LIST_SHAPES[(i + r + SCENE_TREES.index(tree)) % 3]
            what = f"{kind} case {i} under {tree}: {len(b.models)} spheres, {len(b.bvh)} nodes, {w}x{h}, {int(view.cam[0]['bounce_count'])} bounces, {run}, {shape} list"
            planes = CanonPlanes(w, h)
            before = 0
            for n in TARGETS:
                _step(plugin, oracle, view, planes, before, n, run, shape, [i, n, r], f"{what}, to {n}", fl)
                before = n
            if run == "lds":
                device_state, device_frame = planes.state(), planes.frame()
        # the host entry point at the default residency, straight to the last target: the same bytes
        hs, hf = np.zeros((h, w), REC), np.full((h, w, 4), 7.5, F32)
        st = plugin.node.progressive_sample(view.cam, view.win, w, h, hs, TARGETS[-1], frame=hf)
        assert st["kernel_variant"] == STREAM_FORM and st["scene_in_lds"] == 1, (kind, i, tree, st)
        assert _same(_canon_state(hs), device_state) and _same(_canon(hf).view(np.uint8).reshape(h, w, -1), device_frame), (kind, i, tree, "host")
        _ran(st, fl)
    _DONE.add(("prog scenes", kind, tree))


@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
@pytest.mark.parametrize("kind", list(_SCENES))
def test_progressive_steps_on_randomized_and_wild_scenes(plugin, oracle, kind, tree):
    """Every scene to 1 and on to 3 samples: n, rays and the frame are the oracle's after each step, the step's stats count its own
    share; three residencies of the streaming form and the plain form, the list shape rotating over scenes and runs; the host form."""
    _prog_scenes_run(plugin, oracle, kind, tree)


# ---- GPU 2(b): boards, the lane pattern chosen through the list ---------------------------------------------------------------------------------

BOARD_RUNS = ("lds", "global", "plain")


def _prog_board_run(plugin, oracle, name, tree):
    if ("prog board", name, tree) in _DONE:
        return
    view = _board_view(oracle, name, tree)
    fl = _flavour_of(("board", name, tree), view.b)
    plugin.node.write_buffers(view.b)
    lists = board_lists(view.w, view.h, [len(name), view.w, view.h])
    for which, shape in (("tile", "tile"), ("raster", "raster"), ("a", lists["a"]), ("b", lists["b"])):
        for run in BOARD_RUNS:
            planes = CanonPlanes(view.w, view.h)
            before = 0
            for n in (1, sc.SPP):
                _step(plugin, oracle, view, planes, before, n, run, shape, 0, f"{name} under {tree}, list ({which}), {run}, to {n}", fl)
                before = n
    _DONE.add(("prog board", name, tree))


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("name", list(sc.PURE))
def test_progressive_boards_with_the_lane_pattern_chosen_through_the_list(plugin, oracle, name, tree):
    """Every case of shade_cases.PURE to 1 and on to its 4 samples under its PLOC tree, the median-split tree and the single leaf: null
    lists in tile order (lane l holds what lane l of the frame kernel's tile holds) and in raster order, the placement by lane_of with
    refused entries between, and its reverse."""
    _prog_board_run(plugin, oracle, name, tree)


# ---- GPU 2(c): boards whose records start finished, empty and half-way ----------------------------------------------------------------------

MIXED_T = 4
MIXED_CASES = [(name, tree) for name in LENS_BOARDS for tree in ("ploc", "median3")]


def _kinds(w, h):
    """0: a finished record (n = 4), 1: a zero record, 2: a record at n = 1"""
    return (np.arange(w * h) % 3).reshape(h, w)


def _entries(w, h, order):
    """The pixels of a null list's entries in launch order (brt_progressive.hip pixel_of); -1: a pad."""
    if order == 0:
        return np.arange(w * h)
    out = []
    for tile in range(((w + 7) // 8) * ((h + 7) // 8)):
        ty, tx = divmod(tile, (w + 7) // 8)
        for t in range(64):
            px, py = tx * 8 + (t & 7), ty * 8 + (t >> 3)
            out.append(py * w + px if px < w and py < h else -1)
    return np.array(out)


def test_every_wave_of_a_mixed_record_board_holds_all_three_kinds():
    for name, tree in MIXED_CASES:
        _, _, _, _, w, h = _board(name, tree)
        kinds = _kinds(w, h).reshape(-1)
        for order in (0, 1):
            entries = _entries(w, h, order)
            for at in range(0, entries.size, 64):
                wave = entries[at:at + 64]
                wave = wave[wave >= 0]
                if wave.size:
                    assert set(kinds[wave].tolist()) == {0, 1, 2}, (name, order, at)
    assert np.array_equal(np.sort(_entries(9, 7, 1)[_entries(9, 7, 1) >= 0]), np.arange(63)) and _entries(9, 7, 1).size == 128


def _mixed_run(plugin, oracle, name, tree):
    if ("mixed", name, tree) in _DONE:
        return
    view = _board_view(oracle, name, tree)
    w, h = view.w, view.h
    fl = _flavour_of(("board", name, tree), view.b)
    plugin.node.write_buffers(view.b)
    kinds = _kinds(w, h)
    rays_1, rays_t = (view.want(n)[1].astype(np.int64) for n in (1, MIXED_T))
    for k, (flags, variant) in enumerate(FORMS):
        at_1, at_t = Planes(w, h), Planes(w, h)
        at_1.sample(plugin, view.cam, view.win, 1, flags=flags)
        at_t.sample(plugin, view.cam, view.win, MIXED_T, flags=flags)
        state = np.zeros((h, w), REC)
        state[kinds == 0] = at_t.state()[kinds == 0]
        state[kinds == 2] = at_1.state()[kinds == 2]
        planes = CanonPlanes(w, h, state=state)
        with plugin.tuning(BRT_PROGRESSIVE_ORDER=k):
            st = planes.sample(plugin, view.cam, view.win, MIXED_T, flags=flags)
        what = (name, tree, variant)
        assert st["kernel_variant"] == variant and st["reserved"] == 0, (what, st)
        assert st["paths"] == MIXED_T * int((kinds == 1).sum()) + (MIXED_T - 1) * int((kinds == 2).sum()), (what, st)
        assert st["rays"] == int(rays_t[kinds != 0].sum() - rays_1[kinds == 2].sum()), (what, st)
        got = planes.state()
        assert _same(got[kinds == 0], _canon_state(state)[kinds == 0]), what          # the finished records: byte-identical
        assert _same(got, _canon_state(at_t.state())), what                           # the whole state: a run straight to 4
        _check_step(oracle, view, planes, MIXED_T, what)                              # n, rays, every value of the frame stored
        assert np.array_equal(planes.frame(), _bytes(oracle, view.want(MIXED_T)[0], planes.fmt)), what
        _ran(st, fl)
    _DONE.add(("mixed", name, tree))


@pytest.mark.gpu
@pytest.mark.parametrize("name,tree", MIXED_CASES)
def test_progressive_boards_with_mixed_records(plugin, oracle, name, tree):
    """Target 4 on a state whose pixel k holds a finished record (k % 3 == 0), a zero record (1) or the record at one sample (2): the
    finished records leave their lanes idle from the first claim, so the other pixels land on other lanes than in a whole-frame run.
    The finished records are untouched and their values stored, the state is that of a run straight to 4, the frame is the oracle's,
    paths and rays count only the samples run.  Streaming form in raster order, plain form in tile order."""
    _mixed_run(plugin, oracle, name, tree)


# ---- GPU 2(d): the moments under hostile shading ----------------------------------------------------------------------------------------------

MOMENT_BOARDS = ("colours_open", "ladder2_enclosed", "lottery_open")
_NON_FINITE = {}


def _moments_run(plugin, oracle, name):
    if name in _NON_FINITE:
        return
    view = _board_view(oracle, name, "median3")
    w, h = view.w, view.h
    fl = _flavour_of(("board", name, "median3"), view.b)
    plugin.node.write_buffers(view.b)
    planes = Planes(w, h)
    pinhole = brt.lens(0.0)
    want = np.zeros((h, w), REC)
    for step in range(1, 5):
        before = planes.state()
        entries = np.zeros(w * h, brt.RADIANCE_RAY_DTYPE)
        for p in range(w * h):
            px, py = p % w, p // w
            state = int(before[py, px]["rng"]) if step > 1 else brt.lens_seed(view.win, w, h, px, py)
            o, d, after = brt.lens_ray(view.cam, view.win, pinhole, w, h, px, py, state)
            entries[p]["origin"], entries[p]["direction"], entries[p]["seed"] = o, d, after
        rgb = oracle.radiance(view.b, entries, 1, int(view.cam[0]["bounce_count"]))[0]["rgb"]
        st = planes.sample(plugin, view.cam, view.win, step, flags=FORMS[step % 2][0])
        _ran(st, fl)
        got = planes.state()
        for p in range(w * h):
            want[p // w, p % w] = pr.accumulate(want[p // w, p % w], rgb[p])[0]
        for k in ("sum", "m1", "m2"):
            assert _same(_canon(got[k]), _canon(want[k])), (name, step, k)
        assert np.array_equal(got["n"], want["n"]) and (got["n"] == step).all(), (name, step)
    canon = CanonPlanes(w, h, state=planes.state())
    canon.d_frame[:planes.frame_bytes] = planes.d_frame[:planes.frame_bytes]
    _check_step(oracle, view, canon, 4, (name, "four single samples"))
    last = planes.state()
    _NON_FINITE[name] = int((~np.isfinite(last["sum"]).all(axis=-1) | ~np.isfinite(last["m1"]) | ~np.isfinite(last["m2"])).sum())


@pytest.mark.gpu
def test_progressive_moments_under_hostile_shading(plugin, oracle):
    """One sample per call for four calls on the boards of wild base colours, special roughness and special material fields under the
    median-split tree, as test_progressive.test_moments_are_exact: every step's ray comes from the record's own rng through
    brt.lens_ray, its colour from oracle.radiance at one sample, and sum, m1, m2, n are the restated accumulation (a NaN for a NaN).
    At least one board's records hold a non-finite sum or moment."""
    for name in MOMENT_BOARDS:
        _moments_run(plugin, oracle, name)
    print("records with a non-finite sum or moment:", _NON_FINITE)
    assert max(_NON_FINITE.values()) >= 1, _NON_FINITE


# ---- GPU 2(e) / 3(e): 32-bit descriptors with general leaves ------------------------------------------------------------------------------------

BIG_N, BIG_W, BIG_H = 16383, 33, 17
_BIG = {}


def _big(tree):
    if tree not in _BIG:
        b = big_scene(BIG_N, 7)
        bvh = median_split_bvh(b.models, 3) if tree == "median3" else brt.build_bvh(b.models)
        _BIG[tree] = brt.Buffers(b.models, b.materials, bvh)
    return _BIG[tree]


def _big_view(oracle, tree):
    key = ("big", tree)
    if key not in _VIEWS:
        _VIEWS[key] = CanonView(oracle, _big(tree), lambda n: big_view(BIG_W, BIG_H, spp=n), BIG_W, BIG_H)
    return _VIEWS[key]


def _prog_big_run(plugin, oracle, tree):
    if ("prog big", tree) in _DONE:
        return
    view = _big_view(oracle, tree)
    fl = _flavour_of(("big", tree), view.b)
    assert fl == ("general" if tree == "median3" else "simple") and len(view.b.models) == BIG_N > 16382
    plugin.node.write_buffers(view.b)
    for r, run in enumerate(("lds", "plain")):              # (no knob: a scene of 32-bit descriptors is walked from global memory)
        planes = CanonPlanes(BIG_W, BIG_H)
        before = 0
        for n in (2, 3):
            st = _step(plugin, oracle, view, planes, before, n, run, LIST_SHAPES[(r + n) % 3], [n, r], f"{BIG_N} spheres under {tree}, {run}, to {n}", fl,
                       width=32, in_lds=0)
            assert st["scene_in_lds"] == 0, st
            before = n
    _DONE.add(("prog big", tree))


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["median3", "ploc"])
def test_progressive_steps_under_32_bit_descriptors(plugin, oracle, tree):
    """16 383 spheres at 33x17 to 2 and on to 3 samples, both forms: under three-sphere leaves (k_list_stream<ProgStart, SCENE_GLOBAL,
    false, false> and the plain form's general half) and under the PLOC tree; the scene is walked from global memory."""
    _prog_big_run(plugin, oracle, tree)


# ---- GPU: a general-tree frame with more pixels than the launch has lanes --------------------------------------------------------------------
#
# The streaming launch's grid is the list's lanes rounded up to whole workgroups, capped by the device (plan_stream, brt_api_query.cpp: one
# 1024-thread workgroup per CU with the scene in LDS).  Below the cap every entry is claimed by a lane that has run nothing yet; only above
# it does a lane that has ENDED a pixel take another one, and only then do the fields ProgStart::begin resets (m1, m2, rays) hold a
# former pixel's values.  Every other frame of this file is far below the cap (at most 89x172), so this one case is a large frame:
# randomized scene 16 (58 spheres under a median split with multi-sphere leaves) with its own camera at 704x400 = 281 600 pixels.
# tests/test_progressive.py::test_a_list_longer_than_the_launch_has_lanes is the same case on a simple tree.  Measured on the oracle:
# 2.1 s for the 1-sample frame and its pixel_rays.
REFILL_SCENE, REFILL_SIZE = 16, (704, 400)


def _refill_view(oracle):
    key = ("refill",)
    if key not in _VIEWS:
        b, lvl, cam, win, _, _ = _scene("random", REFILL_SCENE, "ploc")
        _VIEWS[key] = CanonView(oracle, b, _view_at(lvl, cam, win), *REFILL_SIZE)
    return _VIEWS[key]


def test_the_refill_scene_is_a_general_tree_that_bounces(oracle):
    view = _refill_view(oracle)
    assert flavour(view.b) == "general" and view.b.bvh["model_count"].max() >= 2
    assert view.rays_to(1) > 1.2 * view.w * view.h          # (paths of several rays: lanes end their pixels at different times)


@pytest.mark.gpu
def test_progressive_refills_on_a_general_tree(plugin, oracle):
    """To 1 sample with a null list, on a frame that outnumbers the launch's lanes: n, rays and the frame are the oracle's, and the
    records -- m1 and m2 with them -- are bitwise the plain form's, which never refills (and whose moments
    test_progressive_moments_under_hostile_shading holds sample by sample).  Then on to 2 in a shuffled order, records and frame
    against the plain form alone (the oracle's share of a second frame of this size is 3 s; the plain form's continuation on this
    scene is held to the oracle in test_progressive_steps_on_randomized_and_wild_scenes)."""
    from helpers import dev
    view = _refill_view(oracle)
    w, h = view.w, view.h
    plugin.node.write_buffers(view.b)
    stream, plain = CanonPlanes(w, h), CanonPlanes(w, h)
    st = stream.sample(plugin, view.cam, view.win, 1)
    lanes = st["n_workgroups"] * st["threads_per_workgroup"]
    assert st["kernel_variant"] == STREAM_FORM and lanes + 1 < w * h, (st, "the frame must outnumber the launch's lanes")
    assert st["rays"] == view.rays_to(1) and st["paths"] == w * h, st
    _ran(st, "general")
    plain.sample(plugin, view.cam, view.win, 1, flags=FORMS[1][0])
    _check_step(oracle, view, stream, 1, "whole frame, streaming form")
    assert _same(stream.state(), plain.state())
    order = np.random.default_rng(9).permutation(w * h).astype(np.uint32)
    st = stream.sample(plugin, view.cam, view.win, 2, dev(order).data_ptr(), order.size)
    st_plain = plain.sample(plugin, view.cam, view.win, 2, flags=FORMS[1][0])
    assert st["paths"] == w * h and st["rays"] == st_plain["rays"] > w * h, (st, st_plain)
    assert _same(stream.state(), plain.state()) and _same(stream.frame(), plain.frame())
    assert (stream.state()["n"] == 2).all()


# ---- GPU 2(f): the one-call form on general trees -------------------------------------------------------------------------------------------------

ONE_FIRST, ONE_MAX, ONE_RADIUS = 2, 8, 1
ONE_GRID = (0.0125, 0.025, 0.05, 0.1, 0.2, 0.4, 0.8, 1.6)
ONE_SIZE = (48, 27)                                          # of the cover case
ONE_RANDOM = 0                                               # randomized scene 0: a median split with multi-sphere leaves (15 spheres, 52x43)


def _one_call_view(oracle, which):
    key = ("one call", which)
    if key not in _VIEWS:
        if which == "cover":
            w, h = ONE_SIZE
            b = TREES["median3"](cover())
            _VIEWS[key] = CanonView(oracle, b, lambda n: brt.cover_camera(w, h, n, 4), w, h)
        else:
            tree = "ploc" if _flavour_of(("random", ONE_RANDOM, "ploc"), _scene("random", ONE_RANDOM, "ploc")[0]) == "general" else "median3"
            _VIEWS[key] = _scene_view(oracle, "random", ONE_RANDOM, tree)
    return _VIEWS[key]


def _one_call_threshold(oracle, which):
    """A MODEL of the records (progressive_ref.model_counts on per-sample luminances taken from the oracle's prefix frames, as
    progressive_ref.CoverModel takes them): the first threshold of the grid at which the first selection takes some pixels and not all."""
    view = _one_call_view(oracle, which)
    luma = np.zeros((ONE_MAX, view.h, view.w), F32)
    prev = np.zeros((view.h, view.w, 3), np.float64)
    for k in range(1, ONE_MAX + 1):
        with np.errstate(all="ignore"):
            cur = view.want(k)[0][..., :3].astype(np.float64) * k
            c = (cur - prev).astype(F32)
        luma[k - 1] = pr.luma(c[..., 0], c[..., 1], c[..., 2])
        prev = cur
    for thr in ONE_GRID:
        n = pr.model_counts(luma, ONE_FIRST, pr.targets_of(ONE_FIRST, ONE_MAX), thr, ONE_RADIUS)
        share = float((n > ONE_FIRST).mean())
        if 0.05 <= share <= 0.95:
            return thr, share
    return None, None


@pytest.mark.parametrize("which", ["cover", "random"])
def test_the_one_call_threshold_selects_some_pixels_and_not_all(oracle, which):
    view = _one_call_view(oracle, which)
    assert flavour(view.b) == "general"
    thr, share = _one_call_threshold(oracle, which)
    print(f"one-call form, {which}: threshold {thr}, modelled share of pixels selected after the first pass {share}")
    assert thr is not None


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cover", "random"])
def test_progressive_one_call_on_a_general_tree(plugin, oracle, which):
    """brt_render_progressive_device, first 2, max 8, on the cover scene under the median-split tree and on a randomized general-tree
    scene, both forms: every n is 2, 4 or 8, some pixels were selected and not all; every pixel's frame value and rays are the oracle's
    at the pixel's own n; and the state is that of the passes replayed on the host -- test_progressive's steps with the selection taken
    from progressive_ref.classes on the state of the pass before."""
    from helpers import dev
    view = _one_call_view(oracle, which)
    w, h = view.w, view.h
    thr, _ = _one_call_threshold(oracle, which)
    plugin.node.write_buffers(view.b)
    try:
        plugin.set_progressive(ONE_FIRST, ONE_MAX, thr, ONE_RADIUS)
        for flags, variant in FORMS:
            planes = CanonPlanes(w, h)
            st = plugin.node.render_progressive_device(view.cam, view.win, w, h, planes.d_state.data_ptr(), planes.d_frame.data_ptr(), flags=flags)
            state, frame = planes.state(), planes.frame().view(F32).reshape(h, w, 4)
            counts = {int(k): int((state["n"] == k).sum()) for k in np.unique(state["n"])}
            print(f"{which}, variant {st['kernel_variant']}: pixels by n {counts}")
            assert st["kernel_variant"] == variant and set(counts) <= {2, 4, 8} and len(counts) >= 2 and counts.get(2, 0) > 0, (counts, st)
            for n in counts:
                at = state["n"] == n
                want_frame, want_rays = view.want(n)
                assert _same(frame[at], want_frame[at]) and np.array_equal(state["rays"][at], want_rays[at]), (which, variant, n)
            assert st["paths"] == int(state["n"].sum()) and st["rays"] == int(state["rays"].astype(np.int64).sum()), st
            # the passes replayed: the selection is the restated rule on the state of the pass before
            steps = CanonPlanes(w, h)
            steps.sample(plugin, view.cam, view.win, ONE_FIRST, flags=flags)
            for t in pr.targets_of(ONE_FIRST, ONE_MAX):
                picked = np.flatnonzero(pr.classes(steps.state(), t, thr, ONE_RADIUS).reshape(-1)).astype(np.uint32)
                if picked.size:
                    steps.sample(plugin, view.cam, view.win, t, dev(picked).data_ptr(), picked.size, flags=flags)
            assert _same(steps.state(), state) and _same(steps.frame(), planes.frame()), (which, variant)
            _ran(st, "general")
    finally:
        plugin.set_progressive()


# ---- GPU 2(g): the table of instantiations that ran ------------------------------------------------------------------------------------------------

CELLS_16 = [("stream", placement, tree, 16) for placement in ("LDS", "LDS_TOP", "GLOBAL") for tree in ("simple", "general")] + [
    ("plain", "-", tree, 16) for tree in ("simple", "general")]
CELLS_32 = [("stream", "GLOBAL", "simple", 32), ("stream", "GLOBAL", "general", 32), ("plain", "-", "simple", 32), ("plain", "-", "general", 32)]


@pytest.mark.gpu
def test_every_progressive_instantiation_ran(plugin, oracle):
    """Every cell of {LDS, LDS_TOP, GLOBAL} x {simple, general} of k_list_stream<ProgStart, .., D16 = true, ..> and both flavours of
    k_list_plain<ProgStart, true> hold at least 10 launches that cast rays; the cells of 32-bit descriptors (global memory, simple and
    general; the plain form) at least one.  (The tests above fill the table; what has not run yet -- this test selected alone -- runs
    here.)"""
    for kind in _SCENES:
        for tree in SCENE_TREES:
            _prog_scenes_run(plugin, oracle, kind, tree)
    for name in sc.PURE:
        for tree in TREES:
            _prog_board_run(plugin, oracle, name, tree)
    for name, tree in MIXED_CASES:
        _mixed_run(plugin, oracle, name, tree)
    for tree in ("median3", "ploc"):
        _prog_big_run(plugin, oracle, tree)
    print("form    placement  tree     descriptors  launches with rays > 0")
    for key in CELLS_16 + CELLS_32:
        print(f"{key[0]:7s} {key[1]:10s} {key[2]:8s} {key[3]:<12d} {_TABLE.get(key, 0)}")
    assert set(_TABLE) <= set(CELLS_16 + CELLS_32), set(_TABLE) - set(CELLS_16 + CELLS_32)
    short = {key: _TABLE.get(key, 0) for key in CELLS_16 if _TABLE.get(key, 0) < MIN_LAUNCHES}
    assert not short, short
    assert _TABLE.get(CELLS_32[0], 0) >= 1 and _TABLE.get(CELLS_32[1], 0) >= 1 and _TABLE.get(CELLS_32[2], 0) + _TABLE.get(CELLS_32[3], 0) >= 1, _TABLE


# ---- GPU 3: the G-buffer kernel -----------------------------------------------------------------------------------------------------------------

HIT_DESC = (brt.GBUFFER_DEPTH_DISTANCE, 0, 2)


def _check_hit_planes(plugin, oracle, key, b, cam, win, w, h, what, host=False):
    """The planes of brt.gbuffer(DEPTH_DISTANCE, 0, 2) without a previous camera on the resident scene `b` against oracle_raycast on b's
    tree, as test_gbuffer.test_hit_planes_on_every_scene_and_size holds them (a NaN for a NaN in the f32 planes)."""
    desc = brt.gbuffer(*HIT_DESC)
    got, st = _device(plugin, cam, win, w, h, desc)
    rays, want, hit = _centre_hits(oracle, key, b, cam, win, w, h)
    ids = got["ids"].reshape(-1)
    assert np.array_equal(_canon(got["depth"]).reshape(-1), _canon(want["t"])), what
    assert np.array_equal(_canon(got["normal"][..., :3]).reshape(-1, 3), _canon(want["normal"])), what
    assert np.array_equal(got["normal"][..., 3].reshape(-1), hit.astype(F32)), what
    assert np.array_equal(ids["material"], want["material"]), what
    assert np.array_equal(ids["status"] & 3, want["status"] & 3), what
    assert not ids["reserved"].any(), what
    # the sphere: the caller's index, which reproduces t and carries the material (the oracle names no sphere; of coincident spheres
    # only the one the walk meets first carries the hit's material unless both do, and then either reproduces t)
    as_hits = np.zeros(len(rays), brt.HIT_DTYPE)
    as_hits["t"], as_hits["sphere"], as_hits["material"], as_hits["status"] = want["t"], ids["sphere"], ids["material"], ids["status"] & 3
    qr.check_spheres(oracle, b.models, rays, as_hits)
    alb = got["albedo"].reshape(-1, 4)
    mm = b.materials[want["material"][hit]]
    assert np.array_equal(_canon(alb[hit, :3]), _canon(mm["base_color"])) and np.array_equal(_canon(alb[hit, 3]), _canon(mm["metallic"])), what
    assert not alb[~hit].view(np.uint32).any(), what
    assert (st["cast"], st["hits"], st["covered"]) == (w * h, int(hit.sum()), 0), (what, st)
    if host:
        planes = plugin.node.render_gbuffer(cam, win, w, h, desc)
        for k in PLANES:
            assert planes[k].tobytes() == got[k].tobytes(), f"{what}: host and device entry points differ in {k}"
    return int(hit.sum())


def _gbuffer_scenes_run(plugin, oracle, kind, tree):
    if ("gbuffer scenes", kind, tree) in _DONE:
        return
    hits = 0
    for i in range(sc.N_SCENES):
        b, _, cam, win, w, h = _scene(kind, i, tree)
        plugin.node.write_buffers(b)
        what = f"{kind} case {i} under {tree}: {len(b.models)} spheres, {len(b.bvh)} nodes, {w}x{h}"
        try:
            plugin.node.render_gbuffer_device(cam, win, w, h, brt.gbuffer(*HIT_DESC))
        except brt.BrtError as e:
            _refusal("gbuffer", kind, i, e)
            continue
        hits += _check_hit_planes(plugin, oracle, (kind, i, tree), b, cam, win, w, h, what, host=i % 4 == 0)
    assert hits > 0
    _DONE.add(("gbuffer scenes", kind, tree))


@pytest.mark.gpu
@pytest.mark.parametrize("tree", SCENE_TREES)
@pytest.mark.parametrize("kind", list(_SCENES))
def test_gbuffer_hit_planes_on_randomized_and_wild_scenes(plugin, oracle, kind, tree):
    """Depth as t, normal, hit flag, sphere, material, the HIT and FRONT_FACE bits, albedo from the caller's material table, zeros where
    nothing was hit, `cast` and `hits`: multi-sphere leaves (an index that named a leaf's first sphere would show in the material,
    the albedo and the sphere), walks the overflow rule cuts short, spheres and boxes that clear the walk flags.  Every fourth scene
    through the host entry point as well."""
    _gbuffer_scenes_run(plugin, oracle, kind, tree)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LENS_BOARDS)
def test_gbuffer_hit_planes_on_a_single_leaf_of_64_spheres(plugin, oracle, name):
    """The boards under one leaf of every sphere: pixel k meets sphere k of material k, the last of the leaf's spheres included."""
    b, _, cam, win, w, h = _board(name, "single_leaf")
    assert len(b.bvh) == 1 and b.bvh[0]["model_count"] == len(b.models) >= 64
    plugin.node.write_buffers(b)
    n_hit = _check_hit_planes(plugin, oracle, ("board", name, "single_leaf"), b, cam, win, w, h, f"{name} under one leaf", host=True)
    got, _ = _device(plugin, cam, win, w, h, brt.gbuffer(*HIT_DESC), planes=("ids",))
    assert n_hit == w * h and np.array_equal(got["ids"]["material"].reshape(-1), np.arange(w * h)), name
    assert np.array_equal(b.models["material_id"][got["ids"]["sphere"].reshape(-1)], np.arange(w * h)), name


# 3(b): the derived planes.  Randomized scenes 16 (a median split with multi-sphere leaves: 58 spheres under 31 nodes, 68x23) and 10 (one
# leaf of 50 spheres, 45x36) under their own trees -- both show spheres, sky and moved spheres (measured on the oracle: hit shares 0.61
# and 0.61, 9 and 49 MOVED pixels) --, and the cover scene under the median split.
DERIVED = {"cover": None, "random16": 16, "random10": 10}
_DERIVED = {}


def _derived_case(oracle, name):
    """A case in the form of test_gbuffer._gpu_case: scene, view, previous camera (gbuffer_cases.orbit), previous models
    (gbuffer_cases.moved_models), the oracle's hits on the tree the GPU walks and the rule on them."""
    if name not in _DERIVED:
        if name == "cover":
            w, h = 96, 54
            b = TREES["median3"](cover())
            lvl, cam, win = gc.view("cover", w, h)
            centre = (0.0, 0.5, 0.0)
        else:
            b, lvl, cam, win, w, h = _scene("random", DERIVED[name], "ploc")
            centre = (0.0, 0.0, 0.0)
        prev_cam = gc.orbit(cam, 0.04, 0.1)
        prev_models, picked = gc.moved_models(b.models, centre)
        cur = _hits_of_rays(oracle, b, _pixel_rays(oracle, cam, win, w, h))
        case = dict(name=name, b=b, lvl=lvl, cam=cam, win=win, w=w, h=h, prev_cam=prev_cam, prev_models=prev_models, picked=picked,
                    oracle_cur=cur)
        case["twin"] = _twin_planes(cam, win, w, h, cur, b.models, prev_cam, prev_models)
        _DERIVED[name] = case
    return _DERIVED[name]


@pytest.mark.parametrize("name", list(DERIVED))
def test_the_derived_plane_cases_on_the_oracle(oracle, name):
    case = _derived_case(oracle, name)
    status = np.array([r["status"] for r in case["twin"]])
    hit = case["oracle_cur"]["hit"]
    moved = int(np.count_nonzero(status & gr.MOVED))
    print(f"{name}: hit share {hit.mean():.3f}, moved {moved}, no-previous {np.count_nonzero(status & gr.NO_PREVIOUS)}")
    assert flavour(case["b"]) == "general" and hit.any() and not hit.all()
    assert case["b"].bvh["model_count"].max() >= 2                                   # (a leaf of several spheres)
    assert moved >= (10 if name == "cover" else 1), moved
    if name == "cover":
        assert set(case["oracle_cur"]["sphere"][(status & gr.MOVED) != 0].tolist()) <= set(case["picked"].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DERIVED))
def test_gbuffer_derived_planes_on_general_trees(plugin, oracle, name):
    """Every plane in the three descriptors of test_gbuffer.DESCS with a previous camera and previous models: against the rule on the
    oracle's hits (test_gbuffer._expected_planes), `moved` and `no_previous` against the twin's status words."""
    case = _derived_case(oracle, name)
    plugin.node.write_buffers(case["b"])
    w, h, cam, win = case["w"], case["h"], case["cam"], case["win"]
    for dm, nf, mf in DESCS:
        desc = brt.gbuffer(dm, nf, mf)
        want = _expected_planes(case, desc)
        got, st = _device(plugin, cam, win, w, h, desc, prev_cam=case["prev_cam"], prev_models=case["prev_models"])
        _assert_planes(got, want, f"{name} {dm}{nf}{mf} device")
        status = want["ids"]["status"]
        assert (st["cast"], st["hits"], st["covered"]) == (w * h, int(case["oracle_cur"]["hit"].sum()), 0), st
        assert (st["moved"], st["no_previous"]) == (int(np.count_nonzero(status & gr.MOVED)), int(np.count_nonzero(status & gr.NO_PREVIOUS))), st
        host = plugin.node.render_gbuffer(cam, win, w, h, desc, prev_camera=case["prev_cam"], prev_models=case["prev_models"])
        for k in PLANES:
            assert host[k].tobytes() == got[k].tobytes(), f"{name} {dm}{nf}{mf}: host and device entry points differ in {k}"


@pytest.mark.gpu
def test_gbuffer_coverage_on_a_general_tree(plugin, oracle):
    """gbuffer_cases.coverage_frame "blocks" on the cover scene under the median-split tree: covered pixels keep their fill bytes, the
    others are the oracle's, `covered` is their count."""
    case = _derived_case(oracle, "cover")
    plugin.node.write_buffers(case["b"])
    w, h, cam, win = case["w"], case["h"], case["cam"], case["win"]
    cov = gc.coverage_frame(w, h, "blocks")
    covered = np.ascontiguousarray(cov[..., 3]).view(np.uint32) == 0
    assert covered.any() and not covered.all() and (covered.reshape(-1) & case["oracle_cur"]["hit"]).any()
    for dm, nf, mf in DESCS:
        desc = brt.gbuffer(dm, nf, mf)
        want = _expected_planes(case, desc)
        got, st = _device(plugin, cam, win, w, h, desc, prev_cam=case["prev_cam"], prev_models=case["prev_models"], cov=cov)
        assert (st["cast"], st["covered"]) == (int((~covered).sum()), int(covered.sum())), st
        assert st["hits"] == int((case["oracle_cur"]["hit"] & ~covered.reshape(-1)).sum()), st
        _assert_planes(got, want, f"coverage {dm}{nf}{mf}", mask=~covered)
        for k in PLANES:
            assert (got[k].view(np.uint8).reshape(h, w, -1)[covered] == COV_FILL).all(), f"plane {k}: a covered pixel was written"


# 3(d): deeper than the stack.  The caterpillar of tests/test_desc32.py at 400 spheres, built the same way (the oracle walks its 24 001-sphere
# one for 2.6 s per 33x17 frame: a median split has no spatial order): the first 40 spheres one behind the other on the view axis,
# chained; the bottom link holds sphere 0 and the root of a median-split tree over the others, 40 levels down.  The slab of
# helpers.big_scene is thin at 360 spheres, so their radii are scaled up until the view shows spheres and sky.
DEEP_N, DEEP_SCALE = 400, 8.0
_DEEP = {}


def _deep():
    if not _DEEP:
        b = big_scene(DEEP_N, 11)
        models = b.models.copy()
        models["radius"] *= F32(DEEP_SCALE)
        o, t = np.array(BIG_VIEW["pos"]), np.array(BIG_VIEW["target"])
        axis = (t - o) / np.linalg.norm(t - o)
        models["position"][:40] = (o + (5.0 + np.arange(40))[:, None] * axis).astype(F32)
        models["radius"][:40] = 0.5
        chain = chain_bvh(models[:40])
        nodes = graft_bvh(chain, len(chain) - 1, median_split_bvh(models[40:], 1), 40)
        _DEEP["deep"] = brt.Buffers(models, b.materials, nodes)
        _DEEP["flat"] = brt.Buffers(models, b.materials, brt.build_bvh(models))
    return _DEEP["deep"], _DEEP["flat"]


def test_the_deep_tree_cuts_walks_short(oracle):
    """validate_scene says more than 40 levels; the centre pixel looks down the chain's axis at a sphere 4.5 away and the oracle sees
    the sky there, because the walk ends at 32 stack entries; on a PLOC tree of the same spheres it sees the sphere."""
    deep, flat = _deep()
    assert brt.validate_scene(deep.models, deep.materials, deep.bvh) > 40 and flavour(deep) == "general"
    _, cam, win = big_view(BIG_W, BIG_H)
    _, want, hit = _centre_hits(oracle, ("deep",), deep, cam, win, BIG_W, BIG_H)
    _, want_flat, hit_flat = _centre_hits(oracle, ("deep flat",), flat, cam, win, BIG_W, BIG_H)
    centre = (BIG_H // 2) * BIG_W + BIG_W // 2
    differ = int((want["t"].view(np.uint32) != want_flat["t"].view(np.uint32)).sum())
    print(f"deep tree: hit share {hit.mean():.3f} (flat {hit_flat.mean():.3f}), {differ} pixels differ from the flat tree")
    assert not hit[centre] and hit_flat[centre] and abs(float(want_flat["t"][centre]) - 4.5) < 0.01
    assert differ >= 1 and hit.any() and not hit.all()


@pytest.mark.gpu
def test_gbuffer_on_a_tree_deeper_than_the_stack(plugin, oracle):
    """The hit planes are the oracle's on that tree, which applies the same overflow rule."""
    deep, _ = _deep()
    _, cam, win = big_view(BIG_W, BIG_H)
    plugin.node.write_buffers(deep)
    _check_hit_planes(plugin, oracle, ("deep",), deep, cam, win, BIG_W, BIG_H, "400-sphere caterpillar", host=True)


@pytest.mark.gpu
def test_gbuffer_under_32_bit_descriptors_with_three_sphere_leaves(plugin, oracle):
    """k_gbuffer<false, false> on 16 383 spheres under the median split of three-sphere leaves, 33x17."""
    b = _big("median3")
    _, cam, win = big_view(BIG_W, BIG_H)
    assert len(b.models) == BIG_N and b.bvh["model_count"].max() == 3
    plugin.node.write_buffers(b)
    n_hit = _check_hit_planes(plugin, oracle, ("big", "median3"), b, cam, win, BIG_W, BIG_H, f"{BIG_N} spheres under three-sphere leaves", host=True)
    assert 0 < n_hit < BIG_W * BIG_H
