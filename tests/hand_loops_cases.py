"""The case table of tests/test_hand_loops_gpu.py, shared by the test module (the parent: it renders the oracle's frames and asserts)
and by tests/tools/hand_loops_child.py (the child process that renders every case in the -DBRT_ASM_COUNT build).

A case is a function -> (buffers, level, camera, window, width, height, knobs), the form of tests/test_interior_step_gpu.py's CASES and
tests/test_leaf_issue_gpu.py's FRAMES, which are taken over by import.  SMALL holds the cases rendered twice per mode (frames 0 and 1
of the view, production and BRT_TUNABLE = 1); LARGE the views big enough for the steady-state instantiation (LEAN 2), whose size
follows from the GPU's CU count and of which the third production frame is recorded.

Row mode (walk_rows_asm, brt_device.h) is reached on purpose by frames of ONE tile, which is one wave: a lane's pixel is
(lane & 7, lane >> 3) (slot_to_pixel, brt_trace.h), every pixel stays in its lane for all of its samples, and walk_run takes the row loop
when at most four rays of the wave walk, none of them unsafe.  So a frame of at most four pixels walks in rows only (R1), a larger one
hands its last walks over from the wide loop (R2), and the lanes and stack columns a row serves are chosen by the frame's shape (R3)."""
import numpy as np

import bevyray_amd as brt
from helpers import big_scene, big_view, chain_bvh, make_buffers, uniforms
from test_interior_step_gpu import CASES as INTERIOR_CASES
from test_interior_step_gpu import _deep_chain, _few, _mat
from test_leaf_issue_gpu import FRAMES as LEAF_FRAMES


def _cover(w, h, spp, bounces, seed=0.5):
    return lambda: (brt.generate_scene(brt.SCENE_COVER, 1), *brt.cover_camera(w, h, spp, bounces, brt.Raytracing.Pure, seed), w, h, {})


# ---- R1: at most four pixels, so at most four rays ever walk: every walk in row mode -----------------------------------------------------
# (seeds: ones for which no ray of the frame is unsafe, i.e. the counting build reports repairing_loop_lanes == (0, 0))
R1 = {f"r1_cover_{w}x{h}": _cover(w, h, 8, 8) for w, h in ((1, 1), (2, 1), (3, 1), (4, 1), (1, 4), (2, 2))}

# ---- R2: more than four pixels: the wide loop suspends its last walks with their stacks in place, row mode finishes them ------------------
R2 = {f"r2_cover_{w}x{h}": _cover(w, h, 4, 8) for w, h in ((5, 1), (8, 1), (8, 8), (13, 9))}


# ---- R3: which source lane a row serves, and its column of the wave's stack array ---------------------------------------------------------
def _deep_chain_column():
    """(a) the deep chain of tests/test_interior_step_gpu.py at 1 x 8, seen along the chain: the pixels are lanes 0, 8, .., 56, so rows
    serve the lane pairs (0, 32), (8, 40), (16, 48), (24, 56), each of which shares a dword of the stack array at different depths."""
    b = _deep_chain({})[0]
    return (b, *uniforms(1, 8, spp=2, bounces=8, pos=(0.0, 0.05, 2.0), target=(0.0, 0.0, -20.0), fov=0.3, seed=0.61), 1, 8, {})


def _rotation(a, b):
    """The rotation matrix that takes the unit vector a to the unit vector b (Rodrigues; a != -b)."""
    v, c = np.cross(a, b), float(np.dot(a, b))
    k = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + k + k @ k / (1.0 + c)


CHAIN_POS, CHAIN_FOV, CHAIN_NEAR_T, CHAIN_STEP, CHAIN_RADIUS, CHAIN_SPP = (0.0, 0.0, 0.0), 0.3, 6.0, 0.3, 0.09, 4


def _chain_view(pixels):
    """An 8 x 8 view.  One pixel: the camera is turned so that the pixel's centre ray runs along -z -- the chain's boxes (all but the
    leaves' are the union box, helpers.chain_bvh) are then a thin column that the other pixels' rays leave before it begins.  Two pixels:
    the camera looks along -z."""
    fwd, up = np.array([0.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0])
    if len(pixels) == 1:
        lvl, cam, win = uniforms(8, 8, spp=CHAIN_SPP, bounces=8, pos=CHAIN_POS, target=tuple(fwd), fov=CHAIN_FOV, seed=0.61)
        d = brt.pixel_ray(cam, win, 8, 8, *pixels[0])[0]["direction"].astype(np.float64)
        r = _rotation(d / np.linalg.norm(d), fwd)
        fwd, up = r @ fwd, r @ up
    return uniforms(8, 8, spp=CHAIN_SPP, bounces=8, pos=CHAIN_POS, target=tuple(float(x) for x in fwd), fov=CHAIN_FOV, seed=0.61,
                    up=tuple(float(x) for x in up))


def chain_pixels_case(pixels, with_chain=True):
    """(b) - (d): 30 spheres under a caterpillar tree (stacks 29 deep) on the centre rays of `pixels` of an 8 x 8 frame -- 30 on the ray of
    one pixel, 15 on each ray of two.  The nearest sphere (radius 0.09 at distance 6: 0.03 rad across) subtends less than the 0.0378 rad
    of a pixel and the rays of different pixels diverge, so every other pixel is sky: the other 63 (62) lanes hold finished or waiting pixel state
    while lane 63 (0; both) walks.  tests/test_hand_loops_gpu.py checks the placement on the oracle.  with_chain = False: the same view
    of one sphere behind the camera."""
    lvl, cam, win = _chain_view(pixels)
    data = []
    if with_chain:
        per = 30 // len(pixels)
        for px, py in pixels:
            ray = brt.pixel_ray(cam, win, 8, 8, px, py)[0]
            o, d = ray["origin"].astype(np.float64), ray["direction"].astype(np.float64)
            d /= np.linalg.norm(d)
            for k in range(per):
                data.append((tuple(float(x) for x in o + d * (CHAIN_NEAR_T + CHAIN_STEP * k)), CHAIN_RADIUS, _mat(len(data))))
        b = make_buffers(data, chain_bvh)
    else:
        b = make_buffers([((0.0, 0.0, 50.0), 0.5, _mat(0))])
    return b, lvl, cam, win, 8, 8, {}


CHAIN_PIXELS = {"r3b_lane63": [(7, 7)], "r3c_lane0": [(0, 0)], "r3d_lanes0_63": [(0, 0), (7, 7)]}
R3 = {"r3a_deep_chain_1x8": _deep_chain_column, **{k: (lambda p=p: chain_pixels_case(p)) for k, p in CHAIN_PIXELS.items()}}


# ---- R4: an unsafe ray in a thin wave ------------------------------------------------------------------------------------------------------
R4_SPP = 4


def _unsafe_camera_ray():
    """A 1 x 1 frame whose camera looks along -z at a diffuse sphere, with `up` parallel to the view direction: `right` is the zero
    vector and every image-plane offset a multiple of (0, 0, -1) (tests/test_parity_gpu.py uses the same camera), so every camera ray is
    (0, 0, -1) exactly -- two zero components, 1 / d infinite -- and fails ray_is_safe.  The bounces leave a diffuse surface in random
    directions and are safe."""
    b = make_buffers([((0.0, 0.0, -5.0), 1.0, brt.StandardMaterial(base_color=(0.7, 0.6, 0.5))),
                      ((1.5, 0.5, -6.0), 1.0, brt.StandardMaterial(base_color=(0.3, 0.6, 0.8))),
                      ((-1.5, -0.5, -4.0), 0.7, brt.StandardMaterial(base_color=(0.8, 0.4, 0.3)))])
    lvl, cam, win = uniforms(1, 1, spp=R4_SPP, bounces=8, pos=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), fov=0.6, seed=0.5)
    cam = cam.copy()
    cam["up"] = (0.0, 0.0, -1.0)
    return b, lvl, cam, win, 1, 1, {}


R4 = {"r4_unsafe_camera_ray_1x1": _unsafe_camera_ray}


# ---- R5: a scene that fits the LDS only without the row scratch -----------------------------------------------------------------------------
# With BRT_BLOCK_THREADS = 1024 and BRT_WG_PER_CU = 1 plan_launch (brt_api_launch.cpp) tries only the {1024, 1} shape and gives up the
# 16 x 320 = 5 120 bytes of row scratch before LDS residency; a 2 x 1 frame carries no drain pool.  R5_N is a sphere count of
# helpers.big_scene under the PLOC tree at which trace_lds_bytes (brt_kernels.hip) fits the 160 KB only without the scratch: a sphere
# costs 128 bytes (a 112-byte pair record and 16 bytes of its own), so the window is 40 spheres wide.  Scanned on an MI355X in steps of
# 4: resident with the scratch up to 984 spheres (lds_bytes 163 792 of 163 840), without it from 988 (159 184) to 1016, the top of the
# tree only from 1020.  1000 is the middle of the window.
R5_KNOBS = {"BRT_BLOCK_THREADS": 1024, "BRT_WG_PER_CU": 1}
R5_N = 1000
R5_SCRATCH_BYTES = 16 * 320


def r5_case(n):
    s = big_scene(n, 11)
    b = brt.Buffers(s.models, s.materials, brt.build_bvh(s.models))
    return (b, *big_view(2, 1, spp=32, bounces=4), 2, 1, dict(R5_KNOBS))       # (32 samples: three of the 64 camera rays hit a sphere)


R5 = {"r5_no_scratch": lambda: r5_case(R5_N), "r5_with_scratch": lambda: r5_case(R5_N - 100)}

# ---- one case with half-sample jobs (16 samples or more: brt_trace.h `slices`) ---------------------------------------------------------------
HALF = {"half_sample_jobs_cover_32x16": _cover(32, 16, 16, 8)}


def _forced_half_sample_jobs():
    """By default only frames of at least six tiles per wave slot of the GPU end in half-sample jobs; BRT_SPLIT_FORCE asks for them on a
    small frame (it does not make a launch knobs-live).  From the second frame of the view on, which runs in the order the first measured."""
    return (*_cover(64, 32, 16, 8)()[:6], {"BRT_SPLIT_FORCE": 32})


HALF_FORCED = {"half_sample_jobs_forced_64x32": _forced_half_sample_jobs}

ROW_CASES = {**R1, **R2, **R3, **R4}
SMALL = {**{f"interior_{k}": v for k, v in INTERIOR_CASES.items()}, **{f"leaf_{k}": v for k, v in LEAF_FRAMES.items()},
         **ROW_CASES, **R5, **HALF, **HALF_FORCED}
MODES = {"production": {}, "knobs_live": {"BRT_TUNABLE": 1}}
SMALL_FRAMES = 2


# ---- the steady-state instantiation on scenes other than the cover scene ----------------------------------------------------------------------
LARGE_SPP, LARGE_BOUNCES, LARGE_FRAMES = 1, 4, 3


def large_size(n_cus):
    """LEAN 2 is chosen when spp * (bounces + 1) < (rays // lanes) // 2 with the rays of the view's last frame and lanes = CUs * 1024
    (brt_api_launch.cpp launch_part).  Every sample traces at least one ray, so at 1 spp a frame of 2 * (bounces + 2) * lanes pixels
    qualifies whatever it shows: 2048 x 1536 at 4 bounces on 256 CUs."""
    pixels = 2 * (LARGE_BOUNCES + 2) * n_cus * 1024
    w = 2048
    return w, -(-pixels // w)


def _large_chain(w, h):
    b = _deep_chain({})[0]
    return (b, *uniforms(w, h, spp=LARGE_SPP, bounces=LARGE_BOUNCES, pos=(0.0, 0.05, 2.0), target=(0.0, 0.0, -20.0), fov=0.3, seed=0.61),
            w, h, {})


def _large_few(w, h):
    b = _few(3)[0]
    return (b, *uniforms(w, h, spp=LARGE_SPP, bounces=LARGE_BOUNCES, pos=(0.0, 0.2, 0.0), target=(0.0, 0.0, -4.0), fov=0.6, seed=0.37),
            w, h, {})


def _large_grid(w, h):
    return (brt.generate_scene(brt.SCENE_STRESS_GRID, 1), *brt.cover_camera(w, h, LARGE_SPP, LARGE_BOUNCES), w, h, {"BRT_FORCE_LDS_TOP": 64})


# name -> (case(w, h), the scene_in_lds its launches must report)
LARGE = {"large_deep_chain": (_large_chain, 1), "large_three_spheres": (_large_few, 1), "large_grid_lds_top": (_large_grid, 2)}
