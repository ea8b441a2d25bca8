"""The case table of tests/test_shade_production_gpu.py, shared by the test module (which renders the oracle's frames and asserts) and by
tests/tools/hand_loops_child.py (the child process that renders the Pure-level cases in the -DBRT_ASM_COUNT build).

A case is a function -> (buffers, level, camera, window, width, height, knobs), the form of tests/hand_loops_cases.py.

The lane board.  A frame of at most 8 x 8 pixels is one tile, which is one wave; the lane of pixel (x, y) is y * 8 + x (slot_to_pixel,
brt_trace.h) and a pixel stays in its lane for all of its samples.  A board puts one sphere of radius 0.09 at distance 6 on the
pixel-centre ray (brt.pixel_ray) of every pixel it wants hit; the camera sits at the origin and looks along -z with fov 0.3, and the
window is 1200 pixels high, so the jitter of a sample is a small fraction of a frame pixel and every sample of a pixel hits the pixel's
own sphere.  The sphere of pixel k = y * w + x carries material k: the first hit of every lane has a material of the table's choosing,
written into the material records directly (roughness and the other fields are not passed through prepare_asset).
  open      bounced rays leave to the sky;
  enclosed  six diffuse spheres of radius 1000 whose near sides form a box of half-width 10 around the origin (neighbours intersect, so
            the box is closed): no sky, every round has a full wave in the sampler, paths run to the bounce limit or are absorbed.  ONE
            sphere around the origin would not do: hit_sphere (raytrace.wgsl:371-383) takes the near root only, so a sphere is never
            hit from inside -- for the same reason front_face is true at every regular hit, and "total internal reflection" is reached
            through ior < 1 on a front face, not from inside a sphere.  (The sky is the only light, so an enclosed frame is 0 or NaN
            everywhere: its witnesses are `rays` and the counting build's lane steps.)

PATTERNS   which lanes need two unit-ball points (D: diffuse), one (M: metal of roughness 0.6), none (G: glass) or have no sphere (-):
           chosen lane sets for ball_loop_asm's masks, open board, 4 samples, 1 and 6 bounces.
LADDERS    even rows D, odd rows M, the column gives the roughness: ball_loop_asm's per-lane `rough` operand, and -- from 1e6 on and for
           the non-finite ones -- bounce rays whose a = dot(d, d) fails walk_run's test while their neighbours' pass.
EDGES      the lottery board (every field from a list of special values), glass of special ior, base colours outside [0, 1].
SMALL_BOARDS  the second ladder and the lottery board at seven frame sizes, enclosed, the roughness-1e6 metal on lane 0: walk_run's
           exit_at = min(walking >> 1, 12) on both sides of 12 with an unsafe ray in the wave.
LEVELS     three boards at FallbackRaster and FallbackRaytraced with seeded raster inputs.
RANDOM / WILD  the 40 randomized scenes of helpers._random_case and 40 of helpers._wild_case.
LARGE      two boards at the size of hand_loops_cases.large_size: the steady-state instantiation (LEAN 2)."""
import functools

import numpy as np

import bevyray_amd as brt
from hand_loops_cases import LARGE_BOUNCES, LARGE_FRAMES, LARGE_SPP, MODES, SMALL_FRAMES, large_size  # noqa: F401  (the child reads them here)
from helpers import _random_case, _wild_case, uniforms

F32 = np.float32
NAN, INF = float("nan"), float("inf")
DISTANCE, RADIUS, FOV, WINDOW_HEIGHT, WALL_RADIUS, WALL_HALF_WIDTH = 6.0, 0.09, 0.3, 1200, 1000.0, 10.0
SPP = 4
METAL_ROUGHNESS = 0.6


def view(w, h, spp, bounces, seed=0.5, level=brt.Raytracing.Pure, window_height=WINDOW_HEIGHT):
    return uniforms(w, h, spp=spp, bounces=bounces, pos=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), fov=FOV, seed=seed, level=level,
                    window_height=window_height)


def lane_of(k, w):
    """The lane of the tile's wave that renders pixel k = y * w + x of a board w pixels wide."""
    return (k // w) * 8 + k % w


# ---- material records ------------------------------------------------------------------------------------------------------------------

def material(base=(0.7, 0.6, 0.5), metallic=0.0, roughness=0.25, ior=1.5, transmission=0.0):
    """One record of brt.MATERIAL_DTYPE with its fields as given (linear colour, roughness not squared)."""
    m = np.zeros(1, brt.MATERIAL_DTYPE)
    m["base_color"], m["metallic"], m["roughness"], m["reflectance"] = base, metallic, roughness, 0.5
    m["ior"], m["specular_transmission"] = ior, transmission
    return m[0]


def lane_colour(k):
    """An ordinary base colour that differs from lane to lane."""
    return (0.2 + 0.7 * ((k * 37) % 64) / 64.0, 0.2 + 0.7 * ((k * 11 + 5) % 64) / 64.0, 0.2 + 0.7 * ((k * 23 + 9) % 64) / 64.0)


def kind_material(kind, k):
    if kind == "D":
        return material(lane_colour(k))
    if kind == "M":
        return material(lane_colour(k), metallic=1.0, roughness=METAL_ROUGHNESS)
    if kind == "G":
        return material((1.0, 1.0, 1.0), transmission=1.0)
    assert kind == "-", kind
    return None


def kind_of(record):
    """The kind of a record of this table as the lottery of shade_landed sees it (metallic and transmission are 0 or 1 here)."""
    if record["metallic"] == 1.0:
        return "M"
    return "G" if record["specular_transmission"] == 1.0 else "D"


# ---- the board -------------------------------------------------------------------------------------------------------------------------

def board(w, h, mats, enclosed, spp=SPP, bounces=6, seed=0.5, level=brt.Raytracing.Pure, window_height=WINDOW_HEIGHT, without=()):
    """mats: one material record (or None: no sphere) per pixel k = y * w + x.  Material w * h is the wall's; it is also that of the one
    sphere behind the camera that a board without any sphere gets (an empty scene is not drawn at all).  without: pixels whose sphere
    is left out after all."""
    assert len(mats) == w * h and w <= 8 and h <= 8
    lvl, cam, win = view(w, h, spp, bounces, seed, level, window_height)
    n = w * h
    materials = np.zeros(n + 1, brt.MATERIAL_DTYPE)
    materials[n] = material((0.5, 0.5, 0.5))
    rows = []
    for k in range(n):
        if mats[k] is None:
            materials[k] = materials[n]
            continue
        materials[k] = mats[k]
        if k in without:
            continue
        ray = brt.pixel_ray(cam, win, w, h, k % w, k // w)[0]
        o, d = ray["origin"].astype(np.float64), ray["direction"].astype(np.float64)
        rows.append((o + d / np.linalg.norm(d) * DISTANCE, RADIUS, k))
    if enclosed:
        for axis in range(3):
            for sign in (-1.0, 1.0):
                centre = [0.0, 0.0, 0.0]
                centre[axis] = sign * (WALL_RADIUS + WALL_HALF_WIDTH)
                rows.append((tuple(centre), WALL_RADIUS, n))
    if not rows:
        rows.append(((0.0, 0.0, 50.0), 0.5, n))
    models = np.zeros(len(rows), brt.MODEL_DTYPE)
    for i, (pos, radius, mid) in enumerate(rows):
        models[i]["position"], models[i]["radius"], models[i]["material_id"] = pos, radius, mid
    return brt.Buffers(models, materials, brt.build_bvh(models)), lvl, cam, win, w, h, {}


# ---- sampler patterns ------------------------------------------------------------------------------------------------------------------

def _lanes(rest, **sets):
    kinds = [rest] * 64
    for kind, lanes in sets.items():
        for lane in lanes:
            kinds[lane] = kind
    return "".join(kinds)


# name -> the kind of lane 0 .. 63
PATTERNS = {
    "all_d": "D" * 64,
    "all_m": "M" * 64,
    "all_g": "G" * 64,
    "all_none": "-" * 64,
    "d_even_m_odd": "DM" * 32,
    "d_low_m_high": "D" * 32 + "M" * 32,
    "m_low_d_high": "M" * 32 + "D" * 32,
    "d0_m63_rest_g": _lanes("G", D=[0], M=[63]),
    "m0_d63_rest_g": _lanes("G", M=[0], D=[63]),
    "d31_m32_rest_g": _lanes("G", D=[31], M=[32]),
    "only_lane0_d": _lanes("-", D=[0]),
    "only_lane63_m": _lanes("-", M=[63]),
    "d31_d32_rest_none": _lanes("-", D=[31, 32]),
}
PATTERN_BOUNCES = (1, 6)
NO_POINT_PATTERNS = ("all_g", "all_none")             # nothing ever needs a unit-ball point: ball_loop_asm's s_cbranch_execz skip


def pattern_case(name, bounces):
    return board(8, 8, [kind_material(kind, k) for k, kind in enumerate(PATTERNS[name])], enclosed=False, bounces=bounces)


# ---- roughness ladders -----------------------------------------------------------------------------------------------------------------
LADDERS = {"ladder1": [0.0, -0.0, 1e-45, 1e-30, 0.5, 1.0, 14.0, 16.0], "ladder2": [1e6, 3e38, INF, -INF, NAN, -1.0, 2.0, 15.9]}
# With the second ladder on all eight rows 25 of the 64 pixels of the open board are NaN (the three non-finite columns), more than the
# 16 a frame may have and still say something: rows 4 - 7 carry finite stand-ins in those columns (still far outside [kLeafALo, kLeafAHi]).
LADDER2_LOWER_ROWS = [1e6, 3e38, 1e4, -1e6, 1e12, -1.0, 2.0, 15.9]
UNSAFE_METAL = dict(metallic=1.0, roughness=1e6)       # a bounce ray of a = dot(d, d) ~ 1e12 |p|^2 > kLeafAHi


def ladder_roughness(name, k, w):
    if name == "ladder2" and k // w >= 4:
        return LADDER2_LOWER_ROWS[(k % w) % 8]
    return LADDERS[name][(k % w) % 8]


def ladder_mats(name, w=8, h=8, lane0_unsafe=False):
    mats = [material(lane_colour(k), metallic=float((k // w) & 1), roughness=ladder_roughness(name, k, w)) for k in range(w * h)]
    if lane0_unsafe:
        mats[0] = material(lane_colour(0), **UNSAFE_METAL)
    return mats


# ---- lottery and glass edges -----------------------------------------------------------------------------------------------------------
def special_values():
    one = F32(1.0)
    return [0.0, -0.0, 1.0, float(np.nextafter(one, F32(0.0))), float(np.nextafter(one, F32(2.0))), 0.5, -1.0, 2.0, NAN, INF, -INF,
            1e-45, 1e-38, 3e38, -3e38, 1e6]


def lottery_mats(w=8, h=8, lane0_unsafe=False):
    s = special_values()
    mats = [material(lane_colour(k), metallic=s[k % 16], transmission=s[(k // 4) % 16], roughness=s[(5 * k + 3) % 16], ior=s[(7 * k + 1) % 16])
            for k in range(w * h)]
    if lane0_unsafe:
        mats[0] = material(lane_colour(0), **UNSAFE_METAL)
    return mats


def glass_mats():
    one = F32(1.0)
    iors = [0.0, -0.0, 0.5, float(np.nextafter(one, F32(0.0))), 1.0, float(np.nextafter(one, F32(2.0))), 1.5, 2.5, -1.5, 1e-38, 1e38, INF, NAN]
    return [material((1.0, 1.0, 1.0), transmission=1.0, ior=iors[k % len(iors)]) for k in range(64)]


WILD_CHANNELS = [-0.5, NAN, INF, -INF, 2.0, -0.0, -3e38, 1e-45]


def colour_mats():
    """Base colours outside [0, 1] on every fifth lane (13 lanes: the frame must stay mostly finite to say anything), D on even lanes and
    M on odd ones; the wild lanes carry one, two or three wild channels."""
    mats = []
    for k in range(64):
        base = list(lane_colour(k))
        if k % 5 == 0:
            j = k // 5
            for c in range(1 + j % 3):
                base[(j + c) % 3] = WILD_CHANNELS[(j + 3 * c) % len(WILD_CHANNELS)]
        mats.append(material(tuple(base), metallic=float(k & 1), roughness=METAL_ROUGHNESS))
    return mats


SPECIAL_MATS = {"ladder1": lambda: ladder_mats("ladder1"), "ladder2": lambda: ladder_mats("ladder2"), "lottery": lottery_mats,
                "glass": glass_mats, "colours": colour_mats}
SPECIAL = {f"{name}_{'enclosed' if enclosed else 'open'}": (lambda make=make, enclosed=enclosed: board(8, 8, make(), enclosed))
           for name, make in SPECIAL_MATS.items() for enclosed in (False, True)}

# ---- smaller boards: walk_run's exit_at on both sides of kWalkExitLanes, an unsafe-making lane in the wave ----------------------------------
SMALL_SIZES = ((1, 1), (2, 1), (3, 1), (5, 1), (8, 3), (5, 5), (8, 8))
SMALL_BOARDS = {}
for _w, _h in SMALL_SIZES:
    SMALL_BOARDS[f"ladder2_{_w}x{_h}"] = lambda w=_w, h=_h: board(w, h, ladder_mats("ladder2", w, h, lane0_unsafe=True), enclosed=True)
    SMALL_BOARDS[f"lottery_{_w}x{_h}"] = lambda w=_w, h=_h: board(w, h, lottery_mats(w, h, lane0_unsafe=True), enclosed=True)
# the boards on which the same launch must step in the repairing loop AND in the hand-written one
MIXED_HANDOVER = tuple(SMALL_BOARDS) + ("ladder2_open", "ladder2_enclosed", "lottery_open", "lottery_enclosed")

PURE = {**{f"pat_{name}_b{b}": (lambda name=name, b=b: pattern_case(name, b)) for name in PATTERNS for b in PATTERN_BOUNCES},
        **SPECIAL, **SMALL_BOARDS}


# ---- levels 1 and 2 --------------------------------------------------------------------------------------------------------------------
def level_case(name, level):
    """-> (case, raster_rgba, raster_depth): the raster colour seeded at random; the reverse-Z depth of a sphere's front at distance
    5.91 is near / 5.91 = 0.0169, and the raster depths are drawn from [0, 0.034), so pixels fall on both sides of the depth compare."""
    mats = {"lottery": lottery_mats, "ladder2": lambda: ladder_mats("ladder2"),
            "d_even_m_odd": lambda: [kind_material(kind, k) for k, kind in enumerate(PATTERNS["d_even_m_odd"])]}[name]()
    rng = np.random.default_rng([7, int(level)])
    raster = rng.random((8, 8, 4), dtype=np.float32)
    depth = rng.random((8, 8), dtype=np.float32) * F32(0.034)
    return board(8, 8, mats, enclosed=False, level=level), raster, depth


LEVEL_BOARDS = ("lottery", "ladder2", "d_even_m_odd")
LEVELS = {f"{name}_level{int(level)}": (lambda name=name, level=level: level_case(name, level))
          for name in LEVEL_BOARDS for level in (brt.Raytracing.FallbackRaster, brt.Raytracing.FallbackRaytraced)}


# ---- randomized and wild scenes --------------------------------------------------------------------------------------------------------
N_SCENES = 40


@functools.lru_cache(maxsize=None)
def random_scenes():
    """The scenes and raster inputs of tests/test_parity_gpu.py::_randomized_scenes -> [(buffers, level, camera, window, w, h, raster, depth)]."""
    rng = np.random.default_rng(2024)
    out = []
    for case in range(N_SCENES):
        b, lvl, cam, win, w, h = _random_case(rng)
        raster = rng.random((h, w, 4), dtype=np.float32) if case % 3 == 0 else None
        depth = (rng.random((h, w), dtype=np.float32) * F32(0.05)) if case % 3 == 0 else None
        out.append((b, lvl, cam, win, w, h, raster, depth))
    return out


WILD_MAX_SPHERES = 400


@functools.lru_cache(maxsize=None)
def wild_scenes():
    """40 draws of helpers._wild_case (the generator of scripts/fuzz_parity.py, every case wild) under the caller's trees, same form;
    level and raster inputs are the generator's own (level Skip and special depth values among them)."""
    rng = np.random.default_rng(2025)
    out = []
    for _ in range(N_SCENES):
        c = _wild_case(rng, wild=True, max_spheres=WILD_MAX_SPHERES, callee_trees=False)
        out.append((c["buffers"], c["level"], c["camera"], c["window"], c["w"], c["h"], c["raster"], c["depth"]))
    return out


# ---- the steady-state instantiation ----------------------------------------------------------------------------------------------------
def _large_board(mats, enclosed):
    """The 8 x 8 board's scene under a camera of the large frame's shape: the 64 spheres fill the view's height (fov 0.3) and the middle
    of its width; the pixels between and beside them see the sky or the walls."""
    def make(w, h):
        b = board(8, 8, mats(), enclosed)[0]
        lvl, cam, win = uniforms(w, h, spp=LARGE_SPP, bounces=LARGE_BOUNCES, pos=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), fov=FOV,
                                 seed=0.37)
        return b, lvl, cam, win, w, h, {}
    return make


# name -> (case(w, h), the scene_in_lds its launches must report)
LARGE = {"large_lottery_open": (_large_board(lottery_mats, False), 1), "large_ladder2_enclosed": (_large_board(lambda: ladder_mats("ladder2"), True), 1)}

# the hand-over boards once more under a five-record top-of-tree tile: the same hand-over in front of walk_wave_top_asm
TOP_KNOBS = {"BRT_FORCE_LDS_TOP": 5}
MIXED_TOP = {f"{name}_top": (lambda name=name: (*PURE[name]()[:6], dict(TOP_KNOBS))) for name in MIXED_HANDOVER}
# what the counting child renders: the Pure-level one-tile cases, two frames per mode, and the large views
SMALL = {**PURE, **MIXED_TOP}
