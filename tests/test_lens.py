"""Lens frames: thin-lens depth of field and orthographic projection (brt_render_lens*, brt_host_lens_*; DESIGN.md "Lens frames").
CPU: the exports, the host twin of the lens rule bitwise against its numpy restatement (tests/lens_ref.py) and, at radius 0, against the C
oracle's first-sample ray; the f32 rule against float64; the optics of the rule in float64; a coverage map of one sphere in and out of
focus; every context-free refusal; a stand-alone sanitizer program; the test lens changes the frame.  GPU: radius 0 bitwise the
oracle's Pure frame; thin-lens and orthographic frames bitwise the host twin's rays shaded by the C oracle; several samples against the
restatement; lists, store formats, an empty sky, the tree's reach, streams, staging buffers, the other entry points, refusals."""
import ctypes as C
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
import lens_ref as lr
import radiance_ref as rr
from bevyray_amd import _lib
from helpers import big_scene, big_view, cover as _cover, dev as _dev, guarded as _guarded, make_buffers, resident_callee_tree, uniforms

npr = lr.npr
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_render_lens_device", "brt_render_lens", "brt_render_lens_pixels_device", "brt_render_lens_pixels", "brt_host_lens_seed",
           "brt_host_lens_ray", "brt_host_lens_origin_bound")
F32 = np.float32
INVALID, UNSUPPORTED, NO_SCENE = -1, -8, -7
W, H = 96, 54
STREAM_FORM, PLAIN_FORM = 34, 35
SCENES = ["cover_callee", "cover_caller", "rtiow", "stress", "big32"]
# the distance of the cover view's target (the origin) from its camera at (13, 2, 3): what the test lens focuses on
COVER_FOCUS = float(np.sqrt(F32(182.0)))
# |f32 rule - float64 rule| over _cases(): the direction's largest component error measures 5.12e-7, the origin's, relative to max(1, |o|), 3.41e-7 (test_the_f32_rule_against_float64 prints
# both; DESIGN.md section 22 records them).  The bounds: four times the measurement, rounded up to one digit.
D_F32_VS_F64 = 3.0e-6
O_F32_VS_F64 = 2.0e-6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ortho(cam):
    c = cam.copy()
    c["projection"] = 1
    return c


@functools.lru_cache(maxsize=None)
def _cases(n=3000, seed=71):
    """n random (camera, window, lens, W, H, px, py, state): positions in [-20, 20]^3, a unit direction, any up, fov 0.1 .. 2; a third
    each pinhole, thin lens (radius 0.01 .. 2, focus 0.5 .. 30) and orthographic (height 0.5 .. 40); frames and windows of 1 .. 2000."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = int(rng.integers(1, 2000)), int(rng.integers(1, 2000))
        _, cam, _ = brt.cover_camera(w, h, 2, 4)
        cam = cam.copy()
        d = rng.normal(size=3)
        cam["position"], cam["direction"], cam["up"] = rng.uniform(-20, 20, 3), d / np.linalg.norm(d), rng.normal(size=3)
        cam["fov"], cam["aspect"] = rng.uniform(0.1, 2.0), rng.uniform(0.3, 3.0)
        win = brt.WindowExtract.extract_component(int(rng.integers(1, 2000)), float(F32(rng.random())))
        mode = i % 3
        lens = brt.lens(float(rng.uniform(0.01, 2.0)) if mode == lr.THIN else 0.0, float(rng.uniform(0.5, 30.0)), float(rng.uniform(0.5, 40.0)))
        if mode == lr.ORTHO:
            cam = _ortho(cam)
        out.append((cam, win, lens, w, h, int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, 2 ** 32))))
    return out


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_in_header_ctypes_rust_and_library():
    header = open(os.path.join(ROOT, "include", "bevyray_amd.h")).read()
    rust = open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    for name in EXPORTS:
        assert f"int32_t {name}(" in header and name in _lib.EXPORTS and f"pub fn {name}(" in rust and f" T {name}\n" in out, name
    assert "typedef struct brt_lens {" in header and "pub struct brt_lens {" in rust
    assert brt.LENS_DTYPE.itemsize == 32 and brt.LENS_DTYPE.names == ("aperture_radius", "focus_distance", "ortho_height", "reserved")
    assert _lib.load().brt_abi_version() == 6


def test_the_host_twin_against_the_restatement():
    """brt_host_lens_ray is lens_ref.sample_ray bit for bit -- origin, direction and the RNG state behind the rule's draws -- and
    brt_host_lens_seed the restated seed, over _cases(): both projections, radius 0 and radius > 0."""
    modes = [0, 0, 0]
    for cam, win, lens, w, h, px, py, state in _cases():
        o, d, after = brt.lens_ray(cam, win, lens, w, h, px, py, state)
        rng = npr.Rng(state)
        wo, wd = lr.sample_ray(cam, win, lens, w, h, px, py, rng)
        assert _same_bits(o, wo) and _same_bits(d, wd) and after == rng.state, (cam, win, lens, w, h, px, py, state, o, wo, d, wd)
        assert brt.lens_seed(win, w, h, px, py) == lr.pixel_seed(win, w, h, px, py)[0]
        modes[lr.mode_of(cam, lens)] += 1
    assert min(modes) >= 900, modes


def test_radius_zero_is_the_oracles_first_sample_ray(oracle):
    """The rule is tied to the C oracle: at radius 0 the first sample of a pixel (the state is the pixel's seed) is
    oracle_first_sample_ray's origin, direction and state."""
    n = 0
    o3, d3, st = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint32(0)
    for cam, win, lens, w, h, px, py, _ in _cases():
        if lr.mode_of(cam, lens) != lr.PINHOLE:
            continue
        assert oracle.lib.oracle_first_sample_ray(cam.ctypes.data, win.ctypes.data, w, h, px, py, C.byref(st), o3, d3) == 0
        o, d, after = brt.lens_ray(cam, win, lens, w, h, px, py, brt.lens_seed(win, w, h, px, py))
        assert _same_bits(o, np.array(tuple(o3), F32)) and _same_bits(d, np.array(tuple(d3), F32)) and after == st.value, (cam, win, w, h, px, py)
        n += 1
    assert n >= 900


def test_the_f32_rule_against_float64():
    worst_d = worst_o = 0.0
    for cam, win, lens, w, h, px, py, state in _cases():
        o, d = lr.sample_ray(cam, win, lens, w, h, px, py, npr.Rng(state))
        o64, d64 = lr.sample_ray64(cam, win, lens, w, h, px, py, npr.Rng(state))
        worst_d = max(worst_d, float(np.abs(d.astype(np.float64) - d64).max()))
        worst_o = max(worst_o, float(np.abs(o.astype(np.float64) - o64).max() / max(1.0, float(np.linalg.norm(o64)))))
    print(f"f32 rule against float64 over {len(_cases())} cases: direction {worst_d:.3e}, origin / max(1, |o|) {worst_o:.3e}")
    assert worst_d <= D_F32_VS_F64 and worst_o <= O_F32_VS_F64


class _Script:
    """An RNG that hands out the given draws"""

    def __init__(self, draws):
        self.draws = list(draws)

    def next_float(self):
        return F32(self.draws.pop(0))


def _cover_lens_view(w=W, h=H, spp=1, bounces=4, radius=0.5, seed=0.5):
    lvl, cam, win = brt.cover_camera(w, h, spp, bounces, seed=seed)
    return lvl, cam, win, brt.lens(radius, COVER_FOCUS)


def test_optics_of_one_jitter_draw_meet_on_the_focus_plane():
    """float64: with the jitter draws fixed, the rays of many disk points pass through one point of the plane at focus_distance along
    the direction, and their lens offsets lie in the plane of right and up within the radius."""
    _, cam, win, lens = _cover_lens_view(radius=0.5)
    c = cam[0]
    cd, cu = c["direction"].astype(np.float64), c["up"].astype(np.float64)
    right = np.cross(cd, cu)
    basis = np.stack([right, cu], axis=1)
    draws = np.random.default_rng(5).random(4000).astype(F32)
    k = n = 0
    while k + 40 < len(draws):
        script = _Script([0.3, 0.9] + list(draws[k:k + 40]))
        before = len(script.draws)
        o, d, l, focus = lr.sample_ray64(cam, win, lens, W, H, 17, 31, script, parts=True)
        k += before - len(script.draws) - 2
        # the ray meets the plane {p: (p - position) . direction = f |direction|^2} in `focus`
        t = (np.dot(focus - o, cd)) / np.dot(d, cd)
        assert np.abs(o + t * d - focus).max() <= 1e-12 * np.abs(focus).max()
        # (`focus` lies on that plane as far as the f32 camera's up and direction are orthogonal)
        assert abs(np.dot(focus - c["position"].astype(np.float64), cd) - float(lens["focus_distance"][0]) * np.dot(cd, cd)) <= 1e-6 * COVER_FOCUS
        ab = np.linalg.lstsq(basis, l, rcond=None)[0]
        assert np.abs(basis @ ab - l).max() <= 1e-14 and ab[0] ** 2 + ab[1] ** 2 <= 0.25 * (1 + 1e-6)      # (the disk test is an f32 one)
        n += 1
    assert n >= 90


def test_the_disk_is_sampled_uniformly():
    """4096 draws: the share of lens offsets inside r / 2 is within 5 sigma of 1 / 4 (sigma = sqrt(4096 * 1/4 * 3/4) = 27.7 draws)."""
    _, cam, win, lens = _cover_lens_view(radius=0.5)
    rng = npr.Rng(12345)
    cd, cu = cam[0]["direction"].astype(np.float64), cam[0]["up"].astype(np.float64)
    basis = np.stack([np.cross(cd, cu), cu], axis=1)
    inside = 0
    for _ in range(4096):
        _, _, l, _ = lr.sample_ray64(cam, win, lens, W, H, 5, 7, rng, parts=True)
        ab = np.linalg.lstsq(basis, l, rcond=None)[0]           # l = a right + b up
        inside += ab[0] ** 2 + ab[1] ** 2 <= 0.25 ** 2
    assert abs(inside - 1024) <= 5 * 27.7, inside


def test_orthographic_directions_and_corner_origins():
    """Every pixel's direction is the same bits; with the jitter at the pixel centre the corner pixels' origins are the closed form
    position +- (1 - 1/W) aspect half right +- (1 - 1/H) half up."""
    _, cam, win, _ = _cover_lens_view()
    cam, lens = _ortho(cam), brt.lens(0.0, 1.0, 7.0)
    c = cam[0]
    want_d = npr.normalize(c["direction"].astype(F32))
    for px, py in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (40, 20)]:
        _, d, _ = brt.lens_ray(cam, win, lens, W, H, px, py, 99 + px)
        assert _same_bits(d, want_d)
        o, _ = lr.sample_ray(cam, win, lens, W, H, px, py, _Script([0.5, 0.5]))
        cd, cu, pos = (c[k].astype(np.float64) for k in ("direction", "up", "position"))
        sx, sy = (2 * (px + 0.5) / W - 1), (1 - 2 * (py + 0.5) / H)
        closed = pos + sx * float(c["aspect"]) * 3.5 * np.cross(cd, cu) + sy * 3.5 * cu
        assert np.abs(o - closed).max() <= O_F32_VS_F64 * max(1.0, np.linalg.norm(closed)), (px, py, o, closed)
    assert (lr.sample_ray(cam, win, lens, W, H, 0, 0, _Script([0.5, 0.5]))[0] != lr.sample_ray(cam, win, lens, W, H, W - 1, H - 1, _Script([0.5, 0.5]))[0]).any()


# -- the coverage map: one sphere of radius R on the axis of a camera at the origin that looks down -z; with no bounce a hit sample is
# black and a miss sample sky, so a pixel's samples that hit are its coverage.  64 x 64 pixels, 16 samples; the view is 10 units high at
# the focus distance F, a pixel 10 / 64 units there, and the circles of radius 2 R - r and 2 R + r on the focus plane differ by 2 r = 6.4
# pixels.
COV_N, COV_SPP, COV_R, COV_r, COV_F = 64, 16, 1.0, 0.5, 10.0


@functools.lru_cache(maxsize=None)
def _coverage(z, radius):
    """-> (64, 64) int: of each pixel's 16 samples, those whose ray (brt_host_lens_ray, the state chained through the rule's draws)
    hits the sphere at (0, 0, -z) (oracle_raycast)."""
    import oracle_loader
    lib = oracle_loader.load().lib
    b = make_buffers([((0.0, 0.0, -z), COV_R, brt.StandardMaterial(base_color=(0.5, 0.5, 0.5)))])
    models, bvh = np.ascontiguousarray(b.models), np.ascontiguousarray(b.bvh)
    _, cam, win = uniforms(COV_N, COV_N, COV_SPP, 0, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 2.0 * math.atan(0.5), 0.37)
    lens = brt.lens(radius, COV_F)
    out7, mat, front = (C.c_float * 7)(), C.c_uint32(0), C.c_int(0)
    fp = C.POINTER(C.c_float)
    cov = np.zeros((COV_N, COV_N), int)
    for py in range(COV_N):
        for px in range(COV_N):
            state = brt.lens_seed(win, COV_N, COV_N, px, py)
            for _ in range(COV_SPP):
                o, d, state = brt.lens_ray(cam, win, lens, COV_N, COV_N, px, py, state)
                lib.oracle_raycast(models.ctypes.data, len(models), bvh.ctypes.data, len(bvh), o.ctypes.data_as(fp), d.ctypes.data_as(fp), out7,
                                   C.byref(mat), C.byref(front))
                cov[py, px] += out7[0] != float(npr.INF)
    cov.setflags(write=False)
    return cov


def _focus_plane_radius():
    """the distance of every pixel centre from the axis on the focus plane, and a pixel's size there"""
    pixel = 10.0 / COV_N
    c = (np.arange(COV_N) + 0.5) * pixel - 5.0
    return np.hypot(c[None, :], c[:, None]), pixel


def _grow(mask):
    out = mask.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out |= np.roll(np.roll(mask, dy, axis=0), dx, axis=1)
    return out


def _out_of_focus_bound(cov):
    """The footprint of the sphere at F / 2 under a lens of radius r.  Seen from a lens point l the sphere's centre lands at -l on the
    focus plane and its silhouette is a circle of radius about 2 R there, so (one pixel of slack each way) every pixel inside 2 R - r is
    touched and none outside 2 R + r.  A pinhole's footprint, the circle of radius about 2 R, lies between those circles as well, so the
    bound also asks that the blur is there: a touched pixel beyond 2 R + r / 2 and a pixel inside 2 R - r / 2 that some sample misses."""
    rho, pixel = _focus_plane_radius()
    touched, full = cov > 0, cov == COV_SPP
    inner = touched[rho <= 2 * COV_R - COV_r - pixel].all()
    outer = not touched[rho >= 2 * COV_R + COV_r + pixel].any()
    blurred = touched[rho >= 2 * COV_R + COV_r / 2].any() and not full[rho <= 2 * COV_R - COV_r / 2].all()
    return inner, outer, blurred


def test_coverage_of_a_sphere_in_focus():
    """z = F: the thin lens touches the pinhole's pixels, give or take one ring of pixels."""
    thin, pin = _coverage(COV_F, COV_r) > 0, _coverage(COV_F, 0.0) > 0
    assert pin.sum() > 100 and not (thin & ~_grow(pin)).any() and not (pin & ~_grow(thin)).any()


def test_coverage_of_a_sphere_out_of_focus():
    assert 2 * COV_r / _focus_plane_radius()[1] >= 6.0
    assert _out_of_focus_bound(_coverage(COV_F / 2, COV_r)) == (True, True, True)
    # ... which is a statement about the lens: the pinhole frame of the same sphere fails it
    assert _out_of_focus_bound(_coverage(COV_F / 2, 0.0)) == (True, True, False)


def _host_calls():
    lib = _lib.load()
    _, cam, win, lens = _cover_lens_view()
    st, seed, bound = C.c_uint32(1), C.c_uint32(0), C.c_float(0)
    o, d = np.zeros(3, F32), np.zeros(3, F32)

    def ray(c=cam, w=win, le=lens, width=W, height=H, px=0, py=0, state=st, oo=o, dd=d):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.brt_host_lens_ray(p(c), p(w), p(le), width, height, px, py, None if state is None else C.byref(state), p(oo), p(dd))

    def bnd(c=cam, le=lens, out=bound):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.brt_host_lens_origin_bound(p(c), p(le), None if out is None else C.byref(out))
    return lib, cam, win, lens, ray, bnd, seed


def test_every_context_free_refusal_names_its_field():
    lib, cam, win, lens, ray, bnd, seed = _host_calls()
    err = lambda: lib.brt_last_error(None).decode()
    assert ray() == 0 and bnd() == 0
    for kw in (dict(c=None), dict(w=None), dict(le=None), dict(state=None), dict(oo=None), dict(dd=None)):
        assert ray(**kw) == INVALID and "null" in err(), kw
    assert bnd(c=None) == INVALID and bnd(le=None) == INVALID and bnd(out=None) == INVALID and "null" in err()
    assert ray(width=0) == INVALID and ray(height=32769) == INVALID and "width/height" in err()
    assert ray(px=W) == INVALID and ray(py=H) == INVALID and "pixel" in err()
    assert lib.brt_host_lens_seed(None, W, H, 0, 0, C.byref(seed)) == INVALID and lib.brt_host_lens_seed(win.ctypes.data, W, H, 0, 0, None) == INVALID
    assert lib.brt_host_lens_seed(win.ctypes.data, W, H, W, 0, C.byref(seed)) == INVALID and lib.brt_host_lens_seed(win.ctypes.data, 0, H, 0, 0, C.byref(seed)) == INVALID

    def refused(c, le, word):
        for rc in (ray(c=c, le=le), bnd(c=c, le=le)):
            assert rc == INVALID and word in err(), (word, err())

    for k in range(5):
        le = lens.copy()
        le["reserved"][0][k] = 1
        refused(cam, le, "reserved")
    for r in (np.nan, -1.0, -1e-45, np.inf, -np.inf):
        refused(cam, brt.lens(r, 1.0), "aperture_radius")
    for f in (np.nan, 0.0, -0.0, -2.0, np.inf):
        refused(cam, brt.lens(0.5, f), "focus_distance")
        assert ray(le=brt.lens(0.0, f)) == 0                       # (not read at radius 0)
    for hgt in (np.nan, 0.0, -1.0, np.inf):
        refused(_ortho(cam), brt.lens(0.0, 1.0, hgt), "ortho_height")
        assert ray(le=brt.lens(0.5, 1.0, hgt)) == 0                # (not read by a perspective camera)
    refused(_ortho(cam), brt.lens(0.25, 1.0, 4.0), "aperture_radius")
    for proj in (2, 3, 0xFFFFFFFF):
        c = cam.copy()
        c["projection"] = proj
        refused(c, lens, "projection_type")
    zero = brt.WindowExtract.extract_component(0, 0.5)
    assert ray(c=_ortho(cam), w=zero, le=brt.lens(0.0, 1.0, 4.0)) == INVALID and "window.height" in err()
    # no context: every render entry point refuses before it reads anything
    for fn, args in ((lib.brt_render_lens_device, (W, H, 4096, None, 0, None)), (lib.brt_render_lens, (W, H, 4096, 0, None)),
                     (lib.brt_render_lens_pixels_device, (W, H, 4096, 4, 8192, None, 0, None)), (lib.brt_render_lens_pixels, (W, H, 4096, 4, 8192, 0, None))):
        assert fn(None, cam.ctypes.data, win.ctypes.data, lens.ctypes.data, *args) == INVALID and "ctx" in err()


def test_the_origin_bound_covers_the_rule():
    """brt_host_lens_origin_bound is at least the 1-norm of every origin the twin produces for the camera and lens, whatever the window,
    frame and pixel; finite for ordinary values; +INF where f32 cannot hold it."""
    rng = np.random.default_rng(3)
    for cam, win, lens, w, h, px, py, state in _cases()[:900]:
        bound = brt.lens_origin_bound(cam, lens)
        assert np.isfinite(bound)
        for _ in range(4):
            o, _, state = brt.lens_ray(cam, win, lens, w, h, int(rng.integers(0, w)), int(rng.integers(0, h)), state)
            assert np.abs(o.astype(np.float64)).sum() <= bound, (cam, lens, o, bound)
    _, cam, _, _ = _cover_lens_view()
    assert brt.lens_origin_bound(cam, brt.lens(0.0)) >= 18.0 and brt.lens_origin_bound(cam, brt.lens(0.0)) < 18.0001
    assert brt.lens_origin_bound(cam, brt.lens(3e38, 1.0)) == np.inf


def test_the_stand_alone_twin_under_sanitizers(tmp_path):
    """tests/tools/lens_twin_main.hip: the rule alone in a program of its own, built with the address and undefined-behaviour sanitizers
    and run on the CPU over special values read from odd addresses."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "lens_twin_main")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "bevyray_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "tools", "lens_twin_main.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr


def test_the_test_lens_changes_the_frame():
    """Non-vacuity, on the restatement: the test lens (the cover camera, radius 0.5, focused on the cover target) changes at least 90 %
    of the pixels of a 24 x 14 frame at 1 spp against the pinhole's."""
    b = _cover()
    w, h = 24, 14
    _, cam, win, lens = _cover_lens_view(w, h, 1, 4)
    sh = npr.Shader(b.models, b.materials, b.bvh, cam[0], win[0], 3)
    thin = np.array([lr.pixel(sh, cam, win, lens, w, h, px, py) for py in range(h) for px in range(w)])
    pin = np.array([lr.pixel(sh, cam, win, brt.lens(0.0), w, h, px, py) for py in range(h) for px in range(w)])
    assert _same_bits(pin.reshape(h, w, 4), npr.render(b.models, b.materials, b.bvh, cam[0], win[0], 3, w, h)[0])      # (the pinhole IS the Pure frame)
    changed = (_bits(thin) != _bits(pin)).any(axis=1).mean()
    print(f"the test lens changes {100 * changed:.1f} % of the pixels")
    assert changed >= 0.9


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _frame_dev(plugin, cam, win, lens, w, h, flags=0, stream=None, out_format=brt.FLAG_OUT_RGBA32F, guard=0):
    """(h, w, 4) of brt_render_lens_device in out_format; with a guard, the bytes behind the frame are checked."""
    import torch
    px_bytes = brt.OUT_PIXEL_BYTES[out_format]
    n = w * h * px_bytes
    buf = _guarded(n, guard, 0xCD)
    plugin.node.render_lens_device(cam, win, lens, w, h, buf.data_ptr(), stream=stream, out_format=out_format, flags=flags)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[n:] == 0xCD).all(), "the guard behind the frame was written"
    dt = {16: F32, 8: np.uint16, 4: np.uint8}[px_bytes]
    return got[:n].view(dt).reshape(h, w, 4).copy()


def _pixels_dev(plugin, cam, win, lens, w, h, pixels, flags=0, stream=None):
    import torch
    pixels = np.ascontiguousarray(pixels, np.uint32)
    d_px = _dev(pixels)
    out = torch.full((max(pixels.size, 1), 4), 7.5, dtype=torch.float32, device="cuda")
    plugin.node.render_lens_pixels_device(cam, win, lens, w, h, d_px.data_ptr(), pixels.size, out.data_ptr(), stream=stream, flags=flags)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:pixels.size]


def _scene(plugin, case, spp=2, bounces=4):
    """-> (Buffers the oracle walks, level, camera, window, expected scene_in_lds of the streaming form) with the scene resident"""
    if case == "big32":
        lvl, cam, win = big_view(W, H, spp, bounces)
        b, win, _ = resident_callee_tree(plugin, big_scene(16383, 7), lvl, cam, win, W, H)
        return b, lvl, cam, win, 0
    kind = {"rtiow": brt.SCENE_RTIOW_FINAL, "stress": brt.SCENE_STRESS_GRID}.get(case, brt.SCENE_COVER)
    b = brt.generate_scene(kind, 1)
    lvl, cam, win = (brt.rtiow_camera if case == "rtiow" else brt.cover_camera)(W, H, spp, bounces)
    if case == "cover_callee":
        b, win, _ = resident_callee_tree(plugin, b, lvl, cam, win, W, H)
    else:
        plugin.node.write_buffers(b)
    return b, lvl, cam, win, 2 if case == "stress" else 1


def _twin_rays(cam, win, lens, w, h, pixels=None):
    """The first sample of every pixel (or of `pixels`) by the host twin -> radiance entries {origin, state behind the rule, direction}"""
    pixels = np.arange(w * h) if pixels is None else pixels
    rays = np.zeros(len(pixels), brt.RADIANCE_RAY_DTYPE)
    for i, p in enumerate(pixels):
        px, py = int(p) % w, int(p) // w
        o, d, state = brt.lens_ray(cam, win, lens, w, h, px, py, brt.lens_seed(win, w, h, px, py))
        rays[i]["origin"], rays[i]["direction"], rays[i]["seed"], rays[i]["user"] = o, d, state, p
    return rays


def _one_sample_frame(oracle, b, rays, bounces):
    """The 1-spp values of the twin's rays: the C oracle's radiance at one sample (sum / f32(1)), alpha 1 -> ((n, 4) f32, rays cast)"""
    res, cnt = oracle.radiance(b, rays, 1, bounces)
    return np.concatenate([res["rgb"], np.ones((len(rays), 1), F32)], axis=1), cnt["rays"]


_TWINS = {}


def _walked(plugin, b):
    """the CPU twin of the tree the last call walked: a callee-built tree at the reach its stats report, else the caller's"""
    reach = plugin.node.last_stats["tree_reach"]
    if reach <= 0:
        return b
    key = (len(b.models), b.models[:64].tobytes(), reach)
    if key not in _TWINS:
        _TWINS[key] = brt.Buffers(b.models, b.materials, brt.build_bvh_sah(b.models, reach))
    return _TWINS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCENES)
def test_radius_zero_is_the_pure_frame(plugin, oracle, case):
    """Perspective, radius 0: the 96 x 54 frame at 2 spp and 4 bounces is oracle.render's bit for bit, ray count included, in both kernel
    forms through the host and the device entry point."""
    b, lvl, cam, win, in_lds = _scene(plugin, case)
    want, cnt = oracle.render(b, lvl, cam, win, W, H)
    lens = brt.lens(0.0, 3.0, 5.0)
    for flags, variant in ((0, STREAM_FORM), (brt.FLAG_KERNEL_SIMPLE, PLAIN_FORM)):
        for entry in ("device", "host"):
            got = _frame_dev(plugin, cam, win, lens, W, H, flags) if entry == "device" else plugin.node.render_lens(cam, win, lens, W, H, flags)
            st = plugin.node.last_stats
            assert _same_bits(got, want), (case, flags, entry)
            assert st["rays"] == cnt["rays"] and st["reserved"] == 0 and st["paths"] == W * H * 2 and st["tree_rebuilt"] == 0, (case, flags, entry, st)
            assert st["kernel_variant"] == variant and st["scene_in_lds"] == (in_lds if variant == STREAM_FORM else 0), (case, st)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCENES)
def test_thin_lens_and_orthographic_frames_at_one_sample(plugin, oracle, case):
    """Radius > 0 and orthographic at 1 spp: every pixel's ray and state from brt_host_lens_ray, its colour from oracle_radiance at one
    sample on the tree the GPU walked; bounces 0, 1 and 8; the streaming form on the device entry point, the plain form on the host's."""
    b, lvl, cam, win, in_lds = _scene(plugin, case, 1, 0)
    big = case == "big32"
    views = {"thin": (cam, brt.lens(0.4 if big else 0.25, 29.0 if big else COVER_FOCUS)), "ortho": (_ortho(cam), brt.lens(0.0, 1.0, 14.0 if big else 5.0))}
    for name, (c, lens) in views.items():
        rays = _twin_rays(c, win, lens, W, H)
        for bounces in (0, 1, 8):
            c = c.copy()
            c["bounce_count"] = bounces
            got = _frame_dev(plugin, c, win, lens, W, H)
            st = dict(plugin.node.last_stats)
            want, n_rays = _one_sample_frame(oracle, _walked(plugin, b), rays, bounces)
            assert _same_bits(got.reshape(-1, 4), want), (case, name, bounces, np.flatnonzero((_bits(got.reshape(-1, 4)) != _bits(want)).any(axis=1))[:8])
            assert st["rays"] == n_rays and st["paths"] == W * H and st["kernel_variant"] == STREAM_FORM and st["scene_in_lds"] == in_lds, (case, name, st)
            assert _same_bits(plugin.node.render_lens(c, win, lens, W, H, brt.FLAG_KERNEL_SIMPLE), got)
            assert plugin.node.last_stats["rays"] == n_rays and plugin.node.last_stats["kernel_variant"] == PLAIN_FORM
        assert (got[..., :3] != got[0, 0, :3]).any()            # (the view shows something)


@pytest.fixture(scope="module")
def restated():
    """The restatement's shader of the cover scene, and per (mode, spp, bounces) the values of a shuffled list of 96 pixels"""
    b = _cover()
    pixels = np.random.default_rng(13).permutation(W * H)[:96].astype(np.uint32)

    @functools.lru_cache(maxsize=None)
    def want(mode, spp, bounces):
        cam, win, lens = _several(mode, spp, bounces)
        sh = npr.Shader(b.models, b.materials, b.bvh, cam[0], win[0], 3)
        return np.array([lr.pixel(sh, cam, win, lens, W, H, int(p) % W, int(p) // W) for p in pixels])
    return b, pixels, want


def _several(mode, spp, bounces):
    _, cam, win, lens = _cover_lens_view(W, H, spp, bounces, radius={"pinhole": 0.0, "thin": 0.5, "ortho": 0.0}[mode])
    return (_ortho(cam), win, brt.lens(0.0, 1.0, 5.0)) if mode == "ortho" else (cam, win, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [0, 1, 8])
@pytest.mark.parametrize("spp", [2, 5])
def test_several_samples_against_the_restatement(plugin, restated, spp, bounces):
    """A shuffled list of 96 pixels through the list export: the samples of a pixel chain one RNG state through the lens rule and the
    shader, as lens_ref.pixel does; a pinhole, a thin lens and an orthographic camera, both forms."""
    b, pixels, want = restated
    plugin.node.write_buffers(b)
    for mode in ("pinhole", "thin", "ortho"):
        cam, win, lens = _several(mode, spp, bounces)
        for flags in (0, brt.FLAG_KERNEL_SIMPLE):
            assert _same_bits(_pixels_dev(plugin, cam, win, lens, W, H, pixels, flags), want(mode, spp, bounces)), (mode, spp, bounces, flags)
        assert _same_bits(plugin.node.render_lens_pixels(cam, win, lens, W, H, pixels), want(mode, spp, bounces))
        assert plugin.node.last_stats["paths"] == 96 * spp


@pytest.fixture(scope="module")
def thin_cover(oracle):
    """The thin-lens view of the cover scene (caller's tree) at 1 spp, 4 bounces and its reference frame: shared, never written"""
    b = _cover()
    _, cam, win, lens = _cover_lens_view(W, H, 1, 4)
    want, n_rays = _one_sample_frame(oracle, b, _twin_rays(cam, win, lens, W, H), 4)
    want.setflags(write=False)
    return b, cam, win, lens, want, n_rays


@pytest.mark.gpu
def test_the_frame_is_its_shuffled_list_scattered_back(plugin, thin_cover):
    b, cam, win, lens, want, n_rays = thin_cover
    plugin.node.write_buffers(b)
    frame = _frame_dev(plugin, cam, win, lens, W, H)
    assert _same_bits(frame.reshape(-1, 4), want) and plugin.node.last_stats["rays"] == n_rays
    order = np.random.default_rng(5).permutation(W * H).astype(np.uint32)
    for flags in (0, brt.FLAG_KERNEL_SIMPLE):
        for got in (_pixels_dev(plugin, cam, win, lens, W, H, order, flags), plugin.node.render_lens_pixels(cam, win, lens, W, H, order, flags)):
            back = np.zeros((W * H, 4), F32)
            back[order] = got
            assert _same_bits(back, frame.reshape(-1, 4)) and plugin.node.last_stats["rays"] == n_rays, flags


@pytest.mark.gpu
def test_list_lengths(plugin, thin_cover):
    """Lengths 1 .. 65, around one workgroup's lane count and around the whole launch's (read from the stats of a long list)"""
    b, cam, win, lens, want, _ = thin_cover
    plugin.node.write_buffers(b)
    rng = np.random.default_rng(19)
    _pixels_dev(plugin, cam, win, lens, W, H, rng.integers(0, W * H, 1 << 20).astype(np.uint32))
    st = plugin.node.last_stats
    group, launch = st["threads_per_workgroup"], st["n_workgroups"] * st["threads_per_workgroup"]
    assert st["kernel_variant"] == STREAM_FORM and launch < (1 << 20)
    lengths = list(range(1, 66)) + [group - 1, group, group + 1, launch - 1, launch, launch + 1, 2 * launch + 63]
    for n in lengths:
        px = rng.integers(0, W * H, n).astype(np.uint32)
        for flags in ((0, brt.FLAG_KERNEL_SIMPLE) if n <= 65 or n >= launch - 1 else (0,)):
            assert _same_bits(_pixels_dev(plugin, cam, win, lens, W, H, px, flags), want[px]), (n, flags)
            assert plugin.node.last_stats["paths"] == n
    assert _pixels_dev(plugin, cam, win, lens, W, H, np.zeros(0, np.uint32)).shape == (0, 4) and plugin.node.last_stats["paths"] == 0


@pytest.mark.gpu
def test_out_of_frame_entries_are_zero_and_counted(plugin, thin_cover):
    b, cam, win, lens, want, _ = thin_cover
    plugin.node.write_buffers(b)
    px = np.random.default_rng(3).integers(0, W * H, 200).astype(np.uint32)
    bad = np.array([0, 7, 63, 64, 130, 199])
    px[bad] = [W * H, W * H + 1, 0xFFFFFFFF, 1 << 31, W * H, W * H + 12345]
    ok = np.ones(200, bool)
    ok[bad] = False
    for flags in (0, brt.FLAG_KERNEL_SIMPLE):
        for got in (_pixels_dev(plugin, cam, win, lens, W, H, px, flags), plugin.node.render_lens_pixels(cam, win, lens, W, H, px, flags)):
            assert plugin.node.last_stats["reserved"] == bad.size and plugin.node.last_stats["paths"] == 200 - bad.size
            assert not _bits(got[bad]).any() and _same_bits(got[ok], want[px[ok]])


@pytest.mark.gpu
def test_radius_zero_lists_are_the_pixel_tracers(plugin):
    """Where the two families of the one kernel pair meet: a shuffled list of all pixels of the 97 x 3 cover frame (2 spp, 1 bounce) with
    two out-of-frame entries, by brt_render_lens_pixels* at aperture radius 0 and by brt_render_pixels*, in both forms through the host and
    the device entry point: the same bits (four zeros at the refused entries), the same refused, path and ray counts, and each family's
    own kernel_variant."""
    import torch
    w, h = 97, 3
    plugin.node.write_buffers(_cover())
    _, cam, win = brt.cover_camera(w, h, 2, 1)
    lens = brt.lens(0.0, 3.0, 5.0)
    px = np.concatenate([np.arange(w * h), [w * h, 0xFFFFFFFF]]).astype(np.uint32)
    px = px[np.random.default_rng(97).permutation(px.size)]
    bad = px >= w * h
    assert px.size == w * h + 2 and bad.sum() == 2 and 0 < np.flatnonzero(bad)[0] and np.flatnonzero(bad)[1] < px.size - 1

    def pinhole_dev(flags):
        d_px = _dev(px)
        out = torch.full((px.size, 4), 7.5, dtype=torch.float32, device="cuda")
        plugin.node.render_pixels_device(cam, win, w, h, d_px.data_ptr(), px.size, out.data_ptr(), flags=flags)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    for flags, form in ((0, 0), (brt.FLAG_KERNEL_SIMPLE, 1)):
        for entry in ("device", "host"):
            got = _pixels_dev(plugin, cam, win, lens, w, h, px, flags) if entry == "device" else plugin.node.render_lens_pixels(cam, win, lens, w, h, px, flags)
            ls = dict(plugin.node.last_stats)
            want = pinhole_dev(flags) if entry == "device" else plugin.node.render_pixels(cam, win, w, h, px, flags)
            ps = dict(plugin.node.last_stats)
            print(f"{entry} flags {flags}: rays {ls['rays']} / {ps['rays']}, paths {ls['paths']} / {ps['paths']}, reserved {ls['reserved']} / {ps['reserved']}")
            assert _same_bits(got, want) and not _bits(got[bad]).any() and (got[~bad, 3] == 1.0).all(), (flags, entry)
            assert ls["reserved"] == ps["reserved"] == 2 and ls["paths"] == ps["paths"] == w * h * 2, (flags, entry, ls, ps)
            assert ls["rays"] == ps["rays"], (flags, entry, ls["rays"], ps["rays"])
            assert ls["kernel_variant"] == STREAM_FORM + form and ps["kernel_variant"] == 32 + form, (flags, entry, ls, ps)


@pytest.mark.gpu
def test_sample_count_zero(plugin, thin_cover):
    b, cam, win, lens, _, _ = thin_cover
    plugin.node.write_buffers(b)
    cam = cam.copy()
    cam["sample_count"] = 0
    for c, le in ((cam, lens), (_ortho(cam), brt.lens(0.0, 1.0, 5.0))):
        for flags in (0, brt.FLAG_KERNEL_SIMPLE):
            got = _frame_dev(plugin, c, win, le, W, H, flags)
            st = plugin.node.last_stats
            assert np.isnan(got[..., :3]).all() and (got[..., 3] == 1.0).all() and st["rays"] == 0 and st["paths"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 37), (37, 1), (97, 3), "window"], ids=lambda s: s if isinstance(s, str) else "%dx%d" % s)
def test_thin_frames_and_a_window_of_another_height(plugin, oracle, size):
    """1 x N, N x 1 and thin frames; and a window twice as high as the target, which sizes the jitter"""
    b = _cover()
    plugin.node.write_buffers(b)
    w, h = (W, H) if size == "window" else size
    _, cam, win, lens = _cover_lens_view(w, h, 1, 4)
    if size == "window":
        same = _one_sample_frame(oracle, b, _twin_rays(cam, win, lens, w, h), 4)[0]
        win = brt.WindowExtract.extract_component(2 * H, 0.5)
    for c, le in ((cam, lens), (_ortho(cam), brt.lens(0.0, 1.0, 5.0))):
        want, n_rays = _one_sample_frame(oracle, b, _twin_rays(c, win, le, w, h), 4)
        for flags in (0, brt.FLAG_KERNEL_SIMPLE):
            assert _same_bits(_frame_dev(plugin, c, win, le, w, h, flags).reshape(-1, 4), want) and plugin.node.last_stats["rays"] == n_rays, (size, flags)
            order = np.random.default_rng(37).permutation(w * h).astype(np.uint32)
            assert _same_bits(_pixels_dev(plugin, c, win, le, w, h, order, flags), want[order])
        if size == "window" and le is lens:
            assert not _same_bits(want, same)                   # (the case is real: the window's height changes the frame)


@pytest.mark.gpu
def test_store_formats_and_the_guard_row(plugin, oracle, thin_cover):
    b, cam, win, lens, want, _ = thin_cover
    plugin.node.write_buffers(b)
    frame = want.reshape(H, W, 4)
    for flags in (0, brt.FLAG_KERNEL_SIMPLE):
        assert _same_bits(_frame_dev(plugin, cam, win, lens, W, H, flags, guard=W * 16), frame)
        for fmt, name in ((brt.FLAG_OUT_RGBA8_UNORM_SRGB, "srgb8"), (brt.FLAG_OUT_RGBA16F, "f16"), (brt.FLAG_OUT_RGBA8_UNORM, "unorm8")):
            got = _frame_dev(plugin, cam, win, lens, W, H, flags, out_format=fmt, guard=W * brt.OUT_PIXEL_BYTES[fmt])
            assert np.array_equal(got, oracle.encode_frame(frame, name)), (flags, name)


@pytest.mark.gpu
def test_an_empty_sky(plugin):
    """The view misses the scene's one sphere: the orthographic frame is one colour, sky_rgb(direction), in every pixel; the thin-lens
    frame at 1 spp is sky_rgb of the twin's directions."""
    b = make_buffers([((0.0, 0.0, 50.0), 1.0, brt.StandardMaterial(base_color=(0.5, 0.5, 0.5)))])
    plugin.node.write_buffers(b)
    _, cam, win = uniforms(W, H, 1, 4, (0.0, 1.0, 0.0), (3.0, 2.5, -10.0), 0.6, 0.5)
    ortho = _ortho(cam)
    for flags in (0, brt.FLAG_KERNEL_SIMPLE):
        got = _frame_dev(plugin, ortho, win, brt.lens(0.0, 1.0, 8.0), W, H, flags)
        sky = rr.sky_rgb(npr.normalize(cam[0]["direction"].astype(F32)))[0]
        assert _same_bits(got[..., :3], np.broadcast_to(sky, (H, W, 3)).copy()) and (got[..., 3] == 1.0).all()
        lens = brt.lens(0.7, 6.0)
        got = _frame_dev(plugin, cam, win, lens, W, H, flags)
        assert _same_bits(got.reshape(-1, 4)[:, :3], rr.sky_rgb(_twin_rays(cam, win, lens, W, H)["direction"])) and plugin.node.last_stats["rays"] == W * H


@pytest.mark.gpu
def test_origins_beyond_the_callee_trees_reach(plugin, oracle):
    """A camera beyond the reach the callee's tree was built for and a lens whose radius pushes the origins further: the call rebuilds
    the tree (stats.tree_rebuilt), to at least what brt_host_lens_origin_bound needs, and the frame is the reference's on the CPU twin of
    that tree; the next call finds the tree as it is."""
    b = _cover()
    _, cam, win = uniforms(W, H, 1, 4, (13.0 * 25, 2.0 * 25, 3.0 * 25), (0.0, 0.0, 0.0), 0.4 / 25, 0.5, far=1.0e5)
    lens = brt.lens(60.0, float(np.sqrt(F32(182.0))) * 25)
    plugin.node.write_buffers(brt.generate_scene(brt.SCENE_RTIOW_FINAL, 1))      # (another scene first: the upload below is a real one)
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    got = _frame_dev(plugin, cam, win, lens, W, H)
    st = dict(plugin.node.last_stats)
    bound = brt.lens_origin_bound(cam, lens)
    assert st["tree_rebuilt"] == 1 and st["tree_reach"] >= brt.tree_reach(b.models, cam)[2] > 0 and plugin.node.query_origin_bound() >= bound, st
    rays = _twin_rays(cam, win, lens, W, H)
    assert np.abs(rays["origin"]).sum(axis=1).max() > np.abs(cam[0]["position"]).sum() + 30.0
    want, n_rays = _one_sample_frame(oracle, _walked(plugin, b), rays, 4)
    assert _same_bits(got.reshape(-1, 4), want) and st["rays"] == n_rays
    got = _frame_dev(plugin, cam, win, lens, W, H, brt.FLAG_KERNEL_SIMPLE)
    st2 = plugin.node.last_stats
    assert st2["tree_rebuilt"] == 0 and st2["tree_reach"] == st["tree_reach"] and _same_bits(got.reshape(-1, 4), want), st2


@pytest.mark.gpu
def test_two_caller_streams_with_an_upload_in_between(plugin, oracle, thin_cover):
    """A lens frame held on stream A, an upload of another scene, a lens frame of that scene on stream B, and a list on the default
    stream under FLAG_CALLER_STREAM: each holds the values of the scene resident when it was called."""
    import torch
    from test_caller_streams import Streams
    b, cam, win, lens, want, _ = thin_cover
    other = brt.generate_scene(brt.SCENE_RTIOW_FINAL, 1)
    want_other = _one_sample_frame(oracle, other, _twin_rays(cam, win, lens, W, H), 4)[0]
    streams = Streams()
    plugin.node.write_buffers(b)
    frames = [torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    px = np.random.default_rng(53).integers(0, W * H, 700).astype(np.uint32)
    d_px, out = _dev(px), torch.full((700, 4), -3.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    streams.hold(streams.a)
    plugin.node.render_lens_device(cam, win, lens, W, H, frames[0].data_ptr(), stream=streams.a.cuda_stream)
    assert plugin.node.last_stats["rays"] == 0                  # (a caller's stream is not synchronised: nothing counted)
    plugin.node.write_buffers(other)                            # (waits for the held frame: uploads wait for the context's lists)
    plugin.node.render_lens_device(cam, win, lens, W, H, frames[1].data_ptr(), stream=streams.b.cuda_stream, flags=brt.FLAG_KERNEL_SIMPLE)
    plugin.node.render_lens_pixels_device(cam, win, lens, W, H, d_px.data_ptr(), 700, out.data_ptr(), stream=0)
    torch.cuda.synchronize()
    assert _same_bits(frames[0].cpu().numpy().reshape(-1, 4), want)
    assert _same_bits(frames[1].cpu().numpy().reshape(-1, 4), want_other) and _same_bits(out.cpu().numpy(), want_other[px])


@pytest.mark.gpu
def test_a_host_call_behind_a_held_one_grows_the_staging_buffers(thin_cover):
    """A device-entry list of 700 is held on a caller's stream; the host entry points then stage a list of 5 000 and a whole frame, which a
    new context has no room for: the buffers are allocated behind the held list.  The held list's output is read last."""
    import torch
    b, cam, win, lens, want, _ = thin_cover
    rng = np.random.default_rng(47)
    held, later = rng.integers(0, W * H, 700).astype(np.uint32), rng.integers(0, W * H, 5000).astype(np.uint32)
    d_held = _dev(held)
    out = torch.full((700, 4), 7.5, dtype=torch.float32, device="cuda")
    sa = torch.cuda.Stream()
    fresh = brt.RaytracePlugin([0])
    try:
        fresh.node.write_buffers(b)
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(20_000_000)                       # (a few ms: the held list starts after the second call has been made)
        fresh.node.render_lens_pixels_device(cam, win, lens, W, H, d_held.data_ptr(), 700, out.data_ptr(), stream=sa.cuda_stream)
        got = fresh.node.render_lens_pixels(cam, win, lens, W, H, later)
        assert _same_bits(got, want[later]) and fresh.node.last_stats["paths"] == 5000
        assert _same_bits(fresh.node.render_lens(cam, win, lens, W, H).reshape(-1, 4), want)                # (grows the output buffer again)
        assert _same_bits(fresh.node.render_lens_pixels(cam, win, lens, W, H, later[:1234], brt.FLAG_KERNEL_SIMPLE), want[later[:1234]])
        torch.cuda.synchronize()
        assert _same_bits(out.cpu().numpy(), want[held])
    finally:
        fresh.close()


@pytest.mark.gpu
def test_the_other_entry_points_are_untouched(plugin, oracle, thin_cover):
    """A plain Pure frame, brt_render_pixels and brt_debug_tile_order give the same bytes before and after lens calls, the oracle's."""
    import torch
    b, cam, win, lens, _, _ = thin_cover
    lvl = brt.cover_camera(W, H, 1, 4)[0]
    plugin.node.write_buffers(b)
    want = oracle.render(b, lvl, cam, win, W, H)[0]
    px = np.random.default_rng(59).integers(0, W * H, 900).astype(np.uint32)
    n = 40
    ray_sum, longest = (np.random.default_rng(61).integers(1, 5000, n).astype(np.uint32) for _ in range(2))

    def others():
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        plugin.node.render_device(lvl, cam, win, W, H, frame.data_ptr())
        order, info = np.zeros(n, np.uint32), np.zeros(4, np.uint32)
        _lib.check(plugin._lib.brt_debug_tile_order(plugin._ctx, ray_sum.ctypes.data, longest.ctypes.data, n, 4, 65536, 8, 0, 0, order.ctypes.data,
                                                    info.ctypes.data), plugin._ctx)
        return frame.cpu().numpy(), plugin.node.render_pixels(cam, win, W, H, px), order, info

    before = others()
    assert _same_bits(before[0], want) and _same_bits(before[1], want.reshape(-1, 4)[px])
    _frame_dev(plugin, cam, win, lens, W, H)
    _frame_dev(plugin, _ortho(cam), win, brt.lens(0.0, 1.0, 5.0), W, H, brt.FLAG_KERNEL_SIMPLE)
    _pixels_dev(plugin, cam, win, lens, W, H, px)
    after = others()
    for x, y in zip(before, after):
        assert _same_bits(x, y)


@pytest.mark.gpu
def test_scene_dependent_refusals_leave_the_context_usable(plugin, thin_cover):
    import torch
    b, cam, win, lens, want, _ = thin_cover
    plugin.node.write_buffers(b)
    lib, ctx = plugin._lib, plugin._ctx
    err = lambda: lib.brt_last_error(ctx).decode()
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    px = np.arange(64, dtype=np.uint32)
    d_px, out = _dev(px), torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    host_frame, host_out = np.zeros((H, W, 4), F32), np.zeros((64, 4), F32)
    p = lambda a: None if a is None else a.ctypes.data

    def dev(c=cam, w=win, le=lens, width=W, height=H, o=frame.data_ptr(), flags=0):
        return lib.brt_render_lens_device(ctx, p(c), p(w), p(le), width, height, o, None, flags, None)

    def lst(c=cam, le=lens, pixels=d_px.data_ptr(), n=64, o=out.data_ptr(), flags=0):
        return lib.brt_render_lens_pixels_device(ctx, p(c), p(win), p(le), W, H, pixels, n, o, None, flags, None)

    def correct():
        assert _same_bits(_frame_dev(plugin, cam, win, lens, W, H).reshape(-1, 4), want)

    for kw in (dict(c=None), dict(w=None), dict(le=None), dict(o=None), dict(width=0), dict(height=32769)):
        assert dev(**kw) == INVALID, kw
    assert lst(pixels=None) == INVALID and lst(o=None) == INVALID and lst(n=0, pixels=None, o=None) == 0
    correct()
    for flags in (brt.FLAG_COUNTERS, brt.FLAG_DENOISE, brt.FLAG_TEMPORAL, brt.FLAG_BLEND_POST, 256):
        assert dev(flags=flags) == INVALID and "flags" in err(), flags
    for flags in (brt.FLAG_OUT_RGBA16F, brt.FLAG_DENOISE):
        assert lst(flags=flags) == INVALID, flags
    assert lib.brt_render_lens(ctx, p(cam), p(win), p(lens), W, H, p(host_frame), brt.FLAG_CALLER_STREAM, None) == INVALID
    assert lib.brt_render_lens(ctx, p(cam), p(win), p(lens), W, H, p(host_frame), brt.FLAG_OUT_RGBA16F, None) == INVALID
    assert lib.brt_render_lens_pixels(ctx, p(cam), p(win), p(lens), W, H, p(px), 64, p(host_out), brt.FLAG_CALLER_STREAM, None) == INVALID
    correct()
    le = lens.copy()
    le["reserved"][0][4] = 7
    assert dev(le=le) == INVALID and "reserved" in err()
    assert dev(le=brt.lens(np.nan, 1.0)) == INVALID and "aperture_radius" in err()
    assert dev(le=brt.lens(0.5, 0.0)) == INVALID and "focus_distance" in err()
    assert dev(c=_ortho(cam), le=brt.lens(0.0, 1.0, 0.0)) == INVALID and "ortho_height" in err()
    assert dev(c=_ortho(cam), le=brt.lens(0.5, 1.0, 4.0)) == INVALID and "aperture_radius" in err()
    three = cam.copy()
    three["projection"] = 2
    assert dev(c=three) == INVALID and "projection_type" in err()
    correct()
    assert dev(le=brt.lens(3e38, 1.0)) == UNSUPPORTED and "bound" in err()          # no f32 bounds those origins
    correct()
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        assert dev() == UNSUPPORTED and lst() == UNSUPPORTED and "policy" in err()
    finally:
        plugin.set_policy(0)
    correct()
    # every other entry point still refuses an orthographic camera
    assert lib.brt_render_pixels_device(ctx, p(_ortho(cam)), p(win), W, H, d_px.data_ptr(), 64, out.data_ptr(), None, 0, None) == UNSUPPORTED
    lvl = brt.cover_camera(W, H, 1, 4)[0]
    with pytest.raises(brt.BrtError):
        plugin.node.render_device(lvl, _ortho(cam), win, W, H, frame.data_ptr())
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any() and not host_frame.any() and not host_out.any()          # no refused call wrote anything
    fresh = brt.RaytracePlugin([0])
    try:
        assert fresh._lib.brt_render_lens_device(fresh._ctx, p(cam), p(win), p(lens), W, H, frame.data_ptr(), None, 0, None) == NO_SCENE
        assert fresh._lib.brt_render_lens_pixels(fresh._ctx, p(cam), p(win), p(lens), W, H, p(px), 64, p(host_out), 0, None) == NO_SCENE
    finally:
        fresh.close()
    correct()
