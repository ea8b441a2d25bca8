"""The production instantiations of k_trace_persistent -- the ones without BRT_FLAG_COUNTERS, which alone compile the hand-written
walk_wave_lds_asm, walk_wave_top_asm, walk_rows_asm and ball_loop_asm, and which bench.py times -- on adversarial materials and chosen
lane patterns: the cases of tests/shade_cases.py (see there for the lane board), bit for bit against the C oracle.

  * CPU: what a case claims is checked on the oracle before anything runs on the GPU -- every pixel of a board hits its own sphere with
    every sample, a pattern's lane sets are what its name says, the special boards' frames are neither all NaN nor all one value, the
    raster depths of the level-1/2 cases fall on both sides of the depth compare.
  * GPU, shipped library (flags = 0): frame and `rays` of every case in production and knobs-live (BRT_TUNABLE = 1), under three
    residencies; three boards at levels 1 and 2; the randomized scenes of the parity tests and the wild scenes of the soak; two boards at
    a frame size that runs in LEAN 2.
  * GPU, -DBRT_ASM_COUNT library (the one tests/test_hand_loops_gpu.py builds; the same child process with this module's case table):
    per production launch the hand-written loops' lane steps against the oracle's counters and the sampler's against the counting frame
    of the same build -- the sampler's draws per lane, where the pixels alone could hide a compensating error --, no sampler iteration
    where no lane needs a point, and the hand-over inside walk_run reached: a launch that steps in the compiler's repairing loop (a
    wave with an unsafe ray) and in the hand-written one.

Every comparison is an equality; a NaN equals a NaN at the same position."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bevyray_amd as brt
import query_ref as qr
import shade_cases as sc
from test_hand_loops_gpu import ROOT, _assert_frame, _assert_identities, counting_lib  # noqa: F401  (counting_lib: the fixture, reused)

# The child's first measured run on an MI355X took 2.6 s (74 one-tile cases, two large views); the limit is ten times that, and at least 60 s.
CHILD_LIMIT_S = 60
RESIDENCIES = {"lds": ({}, 1), "lds_top": ({"BRT_FORCE_LDS_TOP": 5}, 2), "global": ({"BRT_FORCE_GLOBAL_SCENE": 1}, 0)}
_WANT = {}


def _want(oracle, name, make, raster=None, depth=None):
    """The oracle's frame and counters of a case, computed once: (case, frame, counters)."""
    if name not in _WANT:
        case = make()
        b, lvl, cam, win, w, h, _ = case
        frame, cnt = oracle.render(b, lvl, cam, win, w, h, raster_rgba=raster, raster_depth=depth)
        _WANT[name] = (case, np.asarray(frame, np.float32), cnt)
    return _WANT[name]


def _pixels(frame):
    """(pixels that hold a NaN, distinct pixel values) of a frame's colour channels."""
    rgb = np.asarray(frame, np.float32)[..., :3].reshape(-1, 3)
    return int(np.isnan(rgb).any(axis=1).sum()), len({tuple(p) for p in rgb.view(np.uint32).tolist()})


def _first_hit_materials(oracle, case):
    """Per pixel, raster order: the material id the pixel's first sample hits (brt.QUERY_NONE: the sky)."""
    b, _, cam, win, w, h, _ = case
    o, d, _ = oracle.first_sample_rays(cam, win, w, h)
    return qr.expected(oracle, b.models, b.bvh, qr.make_rays(o, d))[0]["material"]


# ---- CPU: the claims of the case table -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window_height", [8, 64, sc.WINDOW_HEIGHT])
def test_every_pixel_of_the_board_hits_its_own_sphere(oracle, window_height):
    """The first-sample ray of pixel k hits the sphere of material k; at 4 samples and 0 bounces all 256 rays hit; without the sphere of
    lane 0, 31, 32 or 63 exactly its pixel's four rays miss.  (Also at the window heights 8 and 64, whose jitter is a whole pixel and an
    eighth of one: the board does not depend on the jitter being small.)"""
    mats = [sc.kind_material("D", k) for k in range(64)]
    case = sc.board(8, 8, mats, enclosed=False, bounces=0, window_height=window_height)
    assert _first_hit_materials(oracle, case).tolist() == list(range(64))
    b, lvl, cam, win, w, h, _ = case
    cnt = oracle.render(b, lvl, cam, win, w, h)[1]
    assert (cnt["hits"], cnt["rays"]) == (64 * sc.SPP, 64 * sc.SPP)
    for k in (0, 31, 32, 63):
        b, lvl, cam, win, w, h, _ = sc.board(8, 8, mats, enclosed=False, bounces=0, window_height=window_height, without=(k,))
        assert oracle.render(b, lvl, cam, win, w, h)[1]["hits"] == 63 * sc.SPP, k


@pytest.mark.parametrize("name", [n for n in sc.SMALL_BOARDS if n.startswith("ladder2")])
def test_every_pixel_of_a_smaller_board_hits_its_own_sphere(oracle, name):
    case = sc.SMALL_BOARDS[name]()
    w, h = case[4:6]
    assert _first_hit_materials(oracle, case).tolist() == list(range(w * h))
    assert sc.kind_of(case[0].materials[0]) == "M" and case[0].materials[0]["roughness"] == np.float32(1e6)


@pytest.mark.parametrize("name", list(sc.PATTERNS))
def test_pattern_lane_sets_are_what_the_table_says(oracle, name):
    """The kind by lane read back from the buffers through the first-sample hit: D, M, G, or no hit at all."""
    case = sc.pattern_case(name, 1)
    hit = _first_hit_materials(oracle, case)
    kinds = "".join("-" if m == brt.QUERY_NONE else sc.kind_of(case[0].materials[m]) for m in hit)
    assert kinds == sc.PATTERNS[name]
    assert [sc.lane_of(k, 8) for k in range(64)] == list(range(64))
    m = [r for r in case[0].materials[:64] if sc.kind_of(r) == "M"]
    assert all(r["roughness"] == np.float32(sc.METAL_ROUGHNESS) for r in m)


@pytest.mark.parametrize("name", list(sc.SPECIAL_MATS))
def test_special_boards_say_something(oracle, name):
    """On the oracle's frame of the open board: at most 16 of the 64 pixels hold a NaN, at least 32 pixels have distinct values (measured
    with this lay-out: ladder1 0 / 64, ladder2 12 / 53, lottery 9 / 57, glass 9 / 56, colours 9 / 64); the first ladder has no NaN pixel.
    The enclosed board of the same materials casts more rays, and where every material is tame (the first ladder) every ray hits."""
    _, frame, cnt = _want(oracle, f"{name}_open", sc.SPECIAL[f"{name}_open"])
    nan, distinct = _pixels(frame)
    print(name, "NaN pixels", nan, "distinct", distinct)
    assert nan <= 16 and distinct >= 32, (nan, distinct)
    if name == "ladder1":
        assert nan == 0
    _, _, cnt_enclosed = _want(oracle, f"{name}_enclosed", sc.SPECIAL[f"{name}_enclosed"])
    assert cnt_enclosed["rays"] > cnt["rays"], (cnt_enclosed, cnt)
    if name == "ladder1":
        assert cnt_enclosed["hits"] == cnt_enclosed["rays"], cnt_enclosed


@pytest.mark.parametrize("name", list(sc.LEVELS))
def test_level_cases_fall_on_both_sides_of_the_depth_compare(oracle, name):
    case, raster, depth = sc.LEVELS[name]()
    _, frame, _ = _want(oracle, name, lambda: case, raster, depth)
    covered = int((frame.view(np.uint32) == raster.view(np.uint32)).all(axis=-1).sum())
    assert 16 <= covered <= 48, covered


def test_wild_scenes_are_small_and_mostly_trace_rays(oracle):
    """40 cases of at most 400 spheres; a scene the library would refuse is known here (brt.validate_scene); at least 15 trace rays (the
    generator draws level Skip and 0 samples too)."""
    scenes = sc.wild_scenes()
    assert len(scenes) == sc.N_SCENES and max(len(s[0].models) for s in scenes) <= sc.WILD_MAX_SPHERES
    wants = [_want_scene(oracle, "wild", i) for i in range(sc.N_SCENES)]
    assert sum(1 for want in wants if want is not None and want[1]["rays"] > 0) >= 15


# ---- GPU, shipped library ------------------------------------------------------------------------------------------------------------------

def _run_modes(plugin, case, want, cnt, what, residency, production_variant, raster=None, depth=None):
    """Two frames of the view in production and two knobs-live under one residency: variant, residency, rays, frame."""
    b, lvl, cam, win, w, h, knobs = case
    res_knobs, in_lds = RESIDENCIES[residency]
    for mode, extra in sc.MODES.items():
        with plugin.tuning(**knobs, **res_knobs, **extra):
            for frame in range(sc.SMALL_FRAMES):
                got = plugin.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, raster_rgba=raster, raster_depth=depth, flags=0)
                st = dict(plugin.node.last_stats)
                key = f"{what}/{residency}/{mode}/{frame}"
                assert (st["kernel_variant"] & 16) if mode == "knobs_live" else st["kernel_variant"] == production_variant, (key, st["kernel_variant"])
                assert st["scene_in_lds"] == in_lds, (key, st["scene_in_lds"])
                assert st["rays"] == cnt["rays"], (key, st["rays"], cnt["rays"])
                _assert_frame(got, want, key)


@pytest.mark.gpu
@pytest.mark.parametrize("residency", list(RESIDENCIES))
@pytest.mark.parametrize("name", list(sc.PURE))
def test_boards_match_the_oracle(plugin, oracle, name, residency):
    """Every pattern, ladder, edge board and smaller board: LEAN 1 (kernel_variant 1) and knobs-live (bit 4), whole scene in LDS
    (walk_wave_lds_asm, walk_rows_asm), a five-record top-of-tree tile (walk_wave_top_asm), everything from global memory."""
    case, want, cnt = _want(oracle, name, sc.PURE[name])
    _run_modes(plugin, case, want, cnt, name, residency, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("residency", ["lds", "lds_top"])
@pytest.mark.parametrize("name", list(sc.LEVELS))
def test_levels_1_and_2_match_the_oracle(plugin, oracle, name, residency):
    """FallbackRaster and FallbackRaytraced with a raster colour and a reverse-Z depth: the no-counters general instantiation
    (kernel_variant 0, the sampler by hand) and its knobs-live twin."""
    case, raster, depth = sc.LEVELS[name]()
    _, want, cnt = _want(oracle, name, lambda: case, raster, depth)
    _run_modes(plugin, case, want, cnt, name, residency, 0, raster, depth)


_SCENES = {"random": sc.random_scenes, "wild": sc.wild_scenes}


def _want_scene(oracle, kind, i):
    """(frame, counters) of scene i of a list by the oracle, once; None where the library refuses the scene."""
    key = (kind, i)
    if key not in _WANT:
        b, lvl, cam, win, w, h, raster, depth = _SCENES[kind]()[i]
        try:
            brt.validate_scene(b.models, b.materials, b.bvh)
        except brt.BrtError:
            _WANT[key] = None
        else:
            frame, cnt = oracle.render(b, lvl, cam, win, w, h, raster_rgba=raster, raster_depth=depth)
            _WANT[key] = (np.asarray(frame, np.float32), cnt)
    return _WANT[key]


@pytest.mark.gpu
@pytest.mark.parametrize("residency", ["lds", "lds_top"])
@pytest.mark.parametrize("kind", list(_SCENES))
def test_randomized_and_wild_scenes_match_the_oracle(plugin, oracle, kind, residency):
    """The 40 scenes of tests/test_parity_gpu.py::_randomized_scenes (fractional metallic and transmission, ior below 1, chains,
    multi-sphere leaves; levels 1 to 3) and 40 wild ones (special radii, positions and material fields, coincident spheres, poisoned
    boxes, camera inside a sphere, window height 0, special seeds, 0 samples, bounce counts past the stack; levels 0 to 3) without
    FLAG_COUNTERS: one production frame and one knobs-live frame each, frame and rays."""
    res_knobs, in_lds = RESIDENCIES[residency]
    for i, (b, lvl, cam, win, w, h, raster, depth) in enumerate(_SCENES[kind]()):
        what = f"{kind} case {i}: {len(b.models)} spheres, {len(b.bvh)} nodes, {w}x{h}, level {int(lvl['level'][0])}, {residency}"
        want = _want_scene(oracle, kind, i)
        for mode, extra in sc.MODES.items():
            with plugin.tuning(**res_knobs, **extra):
                if want is None:
                    with pytest.raises(brt.BrtError):
                        plugin.node.run(lvl, cam, win, w, h, buffers=b, raster_rgba=raster, raster_depth=depth, flags=0)
                    continue
                got = plugin.node.run(lvl, cam, win, w, h, buffers=b, raster_rgba=raster, raster_depth=depth, flags=0)
                st = dict(plugin.node.last_stats)
                if mode == "knobs_live" and int(lvl["level"][0]) != 0:
                    assert st["kernel_variant"] & 16, (what, st["kernel_variant"])
                assert st["rays"] == want[1]["rays"], (what, mode, st["rays"], want[1]["rays"])
                _assert_frame(got, want[0], f"{what} {mode}")


def _n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _want_large(oracle, name):
    w, h = sc.large_size(_n_cus())
    return _want(oracle, name, lambda: sc.LARGE[name][0](w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.LARGE))
def test_steady_state_instantiation_on_the_boards(plugin, oracle, name):
    """1 sample, 4 bounces, a frame of 2 * (bounces + 2) pixels per lane of the GPU (hand_loops_cases.large_size): three frames of the
    view in the shipped library, each with its rays against the oracle, the third in LEAN 2."""
    (b, lvl, cam, win, w, h, knobs), want, cnt = _want_large(oracle, name)
    assert w * h >= 2 * (sc.LARGE_BOUNCES + 2) * _n_cus() * 1024
    with plugin.tuning(**knobs):
        for frame in range(sc.LARGE_FRAMES):
            got = plugin.node.run(lvl, cam, win, w, h, buffers=b if frame == 0 else None, flags=0)
            st = dict(plugin.node.last_stats)
            assert st["rays"] == cnt["rays"], (name, frame, st["rays"], cnt["rays"])
            assert st["scene_in_lds"] == sc.LARGE[name][1], (name, frame, st["scene_in_lds"])
            _assert_frame(got, want, f"{name} frame {frame} variant {st['kernel_variant']}")
    assert st["kernel_variant"] == 2, st["kernel_variant"]


# ---- GPU, counting build -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def child(counting_lib, tmp_path_factory):  # noqa: F811
    """Everything the child saw of this module's cases: records (dict), frames (npz), dir.  Raises if the child ends by a signal, a
    non-zero status or its time limit, so that nothing else that needs it starts on the GPU."""
    out = tmp_path_factory.mktemp("shade_production")
    t0 = time.perf_counter()
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "hand_loops_child.py"), str(out), "shade_cases"],
                          env={**os.environ, "BRT_LIB_PATH": counting_lib}, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    print(f"hand_loops_child.py shade_cases: {time.perf_counter() - t0:.1f} s")
    if proc.returncode != 0:
        raise RuntimeError(f"hand_loops_child.py shade_cases ended with status {proc.returncode}:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}")
    with open(out / "records.json") as f:
        records = json.load(f)
    assert records["lib"] == counting_lib
    return {"records": records, "frames": np.load(out / "frames.npz"), "dir": out}


def _launches(child, name):
    for mode in sc.MODES:
        for frame in range(sc.SMALL_FRAMES):
            key = f"{name}/{mode}/{frame}"
            yield key, mode, frame, child["records"][key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.SMALL))
def test_lane_steps_and_sampler_draws_equal_the_references(child, oracle, name):
    """Per production launch of the counting build: frame, rays, interior and leaf lane steps (hand-written + repairing loop) against
    the oracle, the sampler's lane steps against the compiler-built sampler of the counting frame.  (The *_top cases: the board of the
    same name under a five-record top-of-tree tile.)"""
    case, want, cnt = _want(oracle, name, sc.SMALL[name])
    for key, mode, _, rec in _launches(child, name):
        variant = rec["stats"]["kernel_variant"]
        assert (variant & 16) if mode == "knobs_live" else variant == 1, (key, variant)
        assert rec["stats"]["scene_in_lds"] == (2 if "BRT_FORCE_LDS_TOP" in case[6] else 1), key
        _assert_identities(rec, child["frames"][key], want, cnt, key)


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", sc.PATTERN_BOUNCES)
@pytest.mark.parametrize("name", list(sc.PATTERNS))
def test_sampler_iterations_follow_the_pattern(child, name, bounces):
    """Where no lane ever needs a point (all glass, no sphere) the sampler loop is never entered: no execution, no lane.  Otherwise a lane
    spends at least one iteration per point: at 1 bounce on the open board every sample's camera ray hits its sphere, so the lanes of
    the first frame's iterations are at least (2 |D| + |M|) x samples."""
    kinds = sc.PATTERNS[name]
    for key, _, frame, rec in _launches(child, f"pat_{name}_b{bounces}"):
        ball = list(rec["asm"]["ball"])
        if name in sc.NO_POINT_PATTERNS:
            assert ball == [0, 0], (key, ball)
        else:
            assert ball[0] > 0, (key, ball)
            if bounces == 1 and frame == 0:
                assert ball[1] >= (2 * kinds.count("D") + kinds.count("M")) * sc.SPP, (key, ball)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.MIXED_HANDOVER + tuple(sc.MIXED_TOP))
def test_mixed_hand_over_is_reached(child, name):
    """The same launch steps in the compiler's repairing loop -- a wave that carries an unsafe ray beside safe ones walks there until at
    most exit_at lanes walk -- and in the hand-written loop (walk_wave_lds_asm; walk_wave_top_asm in the *_top cases); on a board of
    more than four pixels the wide loop takes steps of its own (row mode does not account for all of them)."""
    w, h = sc.SMALL[name]()[4:6]
    for key, _, _, rec in _launches(child, name):
        asm = rec["asm"]
        assert asm["repairing_loop_lanes"][0] > 0 and asm["interior"][1] > 0, (key, asm)
        if w * h > 4:
            assert asm["rows_interior_exec"] < asm["interior"][0], (key, asm)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.LARGE))
def test_steady_state_instantiation_lane_steps(child, oracle, name):
    """The third frame of a large view in the counting build: LEAN 2, no row-mode call (it compiles row mode out), the identities."""
    _, want, cnt = _want_large(oracle, name)
    key = f"{name}/production/{sc.LARGE_FRAMES - 1}"
    rec = child["records"][key]
    assert rec["stats"]["kernel_variant"] == 2 and rec["stats"]["scene_in_lds"] == sc.LARGE[name][1], (key, rec["stats"])
    assert rec["asm"]["rows_calls"] == 0 and rec["asm"]["rows_interior_exec"] == 0, (key, rec["asm"])
    _assert_identities(rec, np.load(child["dir"] / f"{name}.npy"), want, cnt, key)
