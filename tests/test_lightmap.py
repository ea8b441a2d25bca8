"""Lightmaps (brt_bake_lightmap*, brt_lightmap_*_device, brt_host_lightmap_*; DESIGN.md "Lightmaps").  CPU: the exports, the direction
table, the host twin of a point's rays on a board of normals and the host dilation against the restatement (tests/lightmap_ref.py) on
synthetic atlases, the f32 rule against float64, every host refusal, buffers at odd addresses, the reference alone on a contact scene,
a stand-alone sanitizer program.  GPU: the three kernels bitwise against the host twins and the restatement; the bake against
brt_radiance_rays_device over the twin's entries plus the restated resolve and dilation and against its own steps, on both trees, both
entry points, both radiance forms and three chunkings; an empty sky; contact darkening; reach; 32-bit descriptors; streams, uploads,
frames and refusals."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
import lightmap_ref as lr
import radiance_ref as rr
from bevyray_amd import _lib
from helpers import big_scene, big_view, cover as _cover, dev as _dev, guarded as _guarded, l1_norm, make_buffers, upload_cover as _upload_cover
from lightmap_ref import assert_texels_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_host_lightmap_directions", "brt_host_lightmap_ray", "brt_host_lightmap_sphere_points", "brt_host_lightmap_dilate",
           "brt_lightmap_rays_device", "brt_lightmap_resolve_device", "brt_lightmap_dilate_device", "brt_bake_lightmap_device",
           "brt_bake_lightmap")
F32 = np.float32
POINT, INFO = brt.LIGHTMAP_POINT_DTYPE, brt.LIGHTMAP_INFO_DTYPE
EMPTY, INVALID_BIT, OUT_OF_REACH = brt.LIGHTMAP_STATUS_EMPTY, brt.QUERY_STATUS_INVALID, brt.QUERY_STATUS_OUT_OF_REACH
INVALID, UNSUPPORTED, NO_SCENE = -1, -8, -7
RGBA16F = brt.FLAG_OUT_RGBA16F
PLAIN, STREAM = 1, 2
# The f32 rule against the same formulas in float64 on 10 000 random unit normals and the 64-direction table, as
# test_the_f32_rule_against_float64 measures and prints them (DESIGN.md section 23 records them): the largest |d32 - d64| per component
# and the largest |t.n|, |bt.n|, |t.bt| of the f32 frame.  The test's bounds: twice each.
DIR_ERROR, T_N, BT_N, T_BT = 2.14e-7, 2.15e-7, 1.98e-7, 1.08e-7
# |mean over the 256-direction table of the linear sky - (A + (2/3) B n_y)| for n = +Y in float64 (test_the_sky_quadrature measures it;
# DESIGN.md section 23); the empty-sky bake may differ from the closed form by that plus 1e-5 for the f32 sqrt-square round trip and sum
SKY_N, SKY_QUADRATURE = 256, 3.64e-6
SIZES = [(1, 1), (1, 7), (7, 1), (17, 9), (64, 64)]                   # (width, height)
PASSES = (0, 1, 3, 64)
ATLASES = ("checker", "single", "none", "all", "special")


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

def _points(rows):
    p = np.zeros(len(rows), POINT)
    for i, (pos, seed, nrm, off) in enumerate(rows):
        p[i]["position"], p[i]["seed"], p[i]["normal"], p[i]["offset"] = pos, seed, nrm, off
    return p


@functools.lru_cache(maxsize=None)
def _board():
    """(points, the status each must get)"""
    nan, inf, o, q = np.nan, np.inf, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0)
    rows = [
        (o, 0, (1, 0, 0), 0.0, 0), (o, 1, (-1, 0, 0), 0.0, 0), (o, 2, (0, 1, 0), 0.0, 0), (o, 3, (0, -1, 0), 0.0, 0),
        (o, 4, (0, 0, 1), 0.0, 0), (o, 0xFFFFFFFF, (0, 0, -1), 0.5, 0), (q, 5, (-0.0, -0.0, 1), 1.0, 0), (q, 6, (-0.0, 1, -0.0), 1.0, 0),
        (q, 7, (1, -0.0, -0.0), -0.0, 0), (q, 8, (6e-4, 0, 8e-4), 1.0, 0), (q, 9, (600, -800, 0), 1.0, 0), (q, 10, (0.3, -0.5, 0.81), 0.25, 0),
        (q, 11, (1e20, 1e20, 1e20), 1.0, INVALID_BIT),            # len2 overflows
        (q, 12, (1e-30, 1e-30, 1e-30), 1.0, INVALID_BIT),         # len2 underflows to 0
        (q, 13, (1e-42, 0, 0), 1.0, INVALID_BIT),                 # a denormal normal
        (q, 14, (nan, 0, 1), 1.0, INVALID_BIT), (q, 15, (0, inf, 1), 1.0, INVALID_BIT), ((nan, 2, 3), 16, (0, 0, 1), 1.0, INVALID_BIT),
        ((1, -inf, 3), 17, (0, 0, 1), 1.0, INVALID_BIT), (q, 18, (0, 0, 1), -1e-3, INVALID_BIT), (q, 19, (0, 0, 1), nan, INVALID_BIT),
        (q, 20, (0, 0, 1), inf, INVALID_BIT),
        (q, 21, (0, 0, 0), 1.0, EMPTY), ((nan, 2, 3), 22, (-0.0, 0, -0.0), nan, EMPTY),                 # EMPTY is looked at first
    ]
    p = _points([r[:4] for r in rows])
    p.setflags(write=False)
    return p, np.array([r[4] for r in rows], np.uint32)


@functools.lru_cache(maxsize=None)
def _dirs(n):
    d = brt.lightmap_directions(n)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _atlas(kind, width, height):
    rng = np.random.default_rng([71, width, height, ATLASES.index(kind)])
    a = np.zeros((height, width, 4), F32)
    a[..., :3] = rng.uniform(0, 4, size=(height, width, 3))
    yy, xx = np.mgrid[0:height, 0:width]
    if kind == "checker":
        a[..., 3] = ((xx // 2 + yy // 2) % 2).astype(F32)
    elif kind == "single":
        a[height - 1, 0, 3] = 1.0
    elif kind == "all":
        a[..., 3] = 1.0
    elif kind == "special":
        a[..., 3] = np.where(rng.uniform(size=(height, width)) < 0.4, F32(1.0), rng.choice(np.array([0.0, -0.0, -1.0, np.nan], F32), size=(height, width)))
        flat = a[..., :3].reshape(-1)
        values = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-42, -1e-42, -0.0]
        for k, i in enumerate(rng.permutation(flat.size)[:max(3, flat.size // 6)]):
            flat[i] = F32(values[(k + width) % len(values)])
        a[0, 0] = (3e38, np.nan, -0.0, 1.0)
        a[..., 3].reshape(-1)[-1] = 0.25                               # (a coverage other than 0, 0.5, 1 is still coverage)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _dilated(kind, width, height, passes, wrap):
    out = lr.dilate(_atlas(kind, width, height), passes, wrap)
    out.setflags(write=False)
    return out


def _twin_rays(points, n_dirs):
    """The point-major list through the library's host twin, one call per entry."""
    pts = np.ascontiguousarray(points, POINT).reshape(-1)
    return np.concatenate([brt.lightmap_ray(p, n_dirs, k) for p in pts for k in range(n_dirs)])


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_in_header_ctypes_rust_and_library():
    header = open(os.path.join(ROOT, "include", "bevyray_amd.h")).read()
    rust = open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    for name in EXPORTS:
        assert f"int32_t {name}(" in header and name in _lib.EXPORTS and f"pub fn {name}(" in rust and f" T {name}\n" in out, name
    assert "#define BRT_LIGHTMAP_STATUS_EMPTY 16u" in header and "pub const BRT_LIGHTMAP_STATUS_EMPTY: u32 = 16;" in rust
    assert "pub struct brt_lightmap_point" in rust and "pub struct brt_lightmap_info" in rust
    assert EMPTY == 16 and EMPTY & (brt.QUERY_STATUS_HIT | brt.QUERY_STATUS_FRONT_FACE | INVALID_BIT | OUT_OF_REACH) == 0
    assert POINT.itemsize == 32 and INFO.itemsize == 8
    assert _lib.load().brt_abi_version() == 6


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1024])
def test_the_direction_table(n):
    got = brt.lightmap_directions(n)
    want = lr.directions64(n)
    w32 = want.astype(F32)
    ulp = np.maximum(np.abs(np.nextafter(w32, F32(np.inf)) - w32), np.abs(w32 - np.nextafter(w32, F32(-np.inf)))).astype(np.float64)
    assert got.shape == (n, 3) and got.dtype == F32 and (np.abs(got.astype(np.float64) - want) <= ulp).all()      # (libm may differ)
    assert (got[:, 2] > 0).all() and np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
    # cosine-weighted: z^2 = 1 - u is uniform, so the mean of z over the table is the midpoint rule of the integral of sqrt(1 - u) = 2/3
    assert abs(got[:, 2].astype(np.float64).mean() - 2.0 / 3.0) <= 0.25 / n
    if n == 1:
        assert np.array_equal(got, np.array([[np.sqrt(0.5), 0.0, np.sqrt(0.5)]], F32))


def test_the_board_has_every_class_of_point():
    pts, want = _board()
    assert np.array_equal(lr.point_status(pts), want)
    assert {0, int(INVALID_BIT), int(EMPTY)} == set(want.tolist())
    with np.errstate(all="ignore"):
        n = pts["normal"]
        len2 = ((n[:, 0] * n[:, 0]).astype(F32) + (n[:, 1] * n[:, 1]).astype(F32)).astype(F32) + (n[:, 2] * n[:, 2]).astype(F32)
    assert np.isinf(len2[12]) and len2[13] == 0 and len2[14] == 0 and pts["normal"][13].any() and pts["normal"][14].any()


@pytest.mark.parametrize("n_dirs", [1, 63, 64, 65, 256])
def test_the_host_ray_is_the_restatement_on_the_board(n_dirs):
    pts, status = _board()
    got = _twin_rays(pts, n_dirs).reshape(len(pts), n_dirs)
    want = lr.make_rays(pts, _dirs(n_dirs)).reshape(len(pts), n_dirs)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    off = status != 0
    assert (got["direction"][off].view(np.uint32) == lr.NAN_WORD).all()
    assert np.array_equal(got["origin"][off].view(np.uint32), np.broadcast_to(pts["position"][off].view(np.uint32)[:, None, :], (off.sum(), n_dirs, 3)))
    assert np.isfinite(got["direction"][~off]).all() and np.isfinite(got["origin"][~off]).all()
    assert np.array_equal(got["user"], np.broadcast_to(np.arange(n_dirs, dtype=np.uint32), got["user"].shape))
    assert np.array_equal(got["seed"][5], lr.seeds(0xFFFFFFFF, n_dirs))                                   # (the seed wraps)
    # what the frame must do where it can be read off: the table's +z is the normal, and the basis is right-handed about it
    d = got["direction"][~off].astype(np.float64)
    n = pts["normal"][~off].astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs((d * n[:, None, :]).sum(axis=2) - _dirs(n_dirs)[None, :, 2]).max() < 1e-6               # d . n = l.z > 0: the hemisphere
    o = got["origin"][~off][:, 0].astype(np.float64)
    assert np.abs(o - (pts["position"][~off] + pts["offset"][~off][:, None].astype(np.float64) * n)).max() < 1e-6


def test_the_f32_rule_against_float64():
    rng = np.random.default_rng(2301)
    v = rng.normal(size=(10000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    pts = np.zeros(10000, POINT)
    pts["normal"] = v.astype(F32)
    assert v[:, 2].min() < -0.999 and v[:, 2].max() > 0.999                                               # (both poles of the basis are near)
    dirs = _dirs(64)
    err = np.abs(lr.directions_of(pts, dirs) - lr.directions_of(pts, dirs, np.float64)).max()
    _, n, t, bt = (x.astype(np.float64) for x in lr.frame(pts))
    tn, btn, tbt = (np.abs((a * b).sum(axis=1)).max() for a, b in ((t, n), (bt, n), (t, bt)))
    print(f"largest |d32 - d64| {err:.3e}; |t.n| {tn:.3e}, |bt.n| {btn:.3e}, |t.bt| {tbt:.3e}")
    assert err <= 2 * DIR_ERROR and tn <= 2 * T_N and btn <= 2 * BT_N and tbt <= 2 * T_BT
    # the library's twin is that f32 rule
    some = pts[::500]
    assert np.array_equal(_twin_rays(some, 64).view(np.uint32), lr.make_rays(some, dirs).view(np.uint32))
    # the float64 frame itself is orthonormal to rounding: the formulas are right, not merely restated alike
    _, n, t, bt = lr.frame(pts, np.float64)
    for a, b, want in ((t, n, 0), (bt, n, 0), (t, bt, 0), (t, t, 1), (bt, bt, 1), (n, n, 1)):
        assert np.abs((a * b).sum(axis=1) - want).max() < 1e-6                                           # (n itself is an f32 vector made unit)
    assert np.abs(np.cross(t, bt) - n).max() < 1e-6


def test_the_sky_quadrature():
    mean, closed = lr.sky_mean64((0.0, 1.0, 0.0), _dirs(SKY_N))
    measured = np.abs(mean - closed).max()
    print(f"float64 restatement, {SKY_N} directions about +Y: largest |mean sky - (A + 2/3 B)| {measured:.3e}")
    assert 0.5 * SKY_QUADRATURE <= measured <= SKY_QUADRATURE                                             # (the figure the GPU test's bound is made from)
    more = lr.sky_mean64((0.0, 1.0, 0.0), _dirs(1024))
    assert np.abs(more[0] - more[1]).max() < measured


@pytest.mark.parametrize("size", SIZES)
def test_the_host_dilate_is_the_restatement(size):
    w, h = size
    for kind in ATLASES:
        src = _atlas(kind, w, h)
        for passes in PASSES:
            for wrap in (False, True):
                got = brt.lightmap_dilate_host(src, passes, wrap)
                want = _dilated(kind, w, h, passes, wrap)
                what = f"{kind} {size} passes {passes} wrap {wrap}"
                assert_texels_equal(got, want, what)
                covered = src[..., 3] > 0
                assert_texels_equal(got[covered], src[covered], what + ": covered texels are copied")
                assert set(np.unique(got[~covered & (got[..., 3] > 0)][:, 3])) <= {F32(0.5)}, what
                if passes == 0 or kind in ("none", "all"):
                    assert_texels_equal(got, src, what + ": nothing to do")
        if w * h > 1:
            assert np.isnan(_dilated("special", w, h, 3, True)).any()
    if size == (17, 9):                                                                                   # the wrap is not vacuous
        assert _dilated("single", w, h, 1, True)[h - 1, w - 1, 3] == 0.5 and _dilated("single", w, h, 1, False)[h - 1, w - 1, 3] == 0.0
        assert np.count_nonzero(_dilated("single", w, h, 3, False)[..., 3] == 0.5) == 15                  # (a 4 x 4 corner less the texel)


def test_64_passes_fill_a_64_x_64_image_from_one_texel():
    src = _atlas("single", 64, 64)                                                                        # the texel (0, 63): a corner
    for dilate in (lambda p, w: _dilated("single", 64, 64, p, w), lambda p, w: brt.lightmap_dilate_host(src, p, w)):
        full = dilate(64, False)
        assert (full[..., 3] > 0).all() and np.count_nonzero(full[..., 3] == 0.5) == 64 * 64 - 1 and np.isfinite(full).all()
        assert np.abs(full[..., :3] - src[63, 0, :3]).max() < 1e-3                                        # (every fill is a mean of copies of it)
    three = _dilated("single", 64, 64, 3, False)
    assert np.count_nonzero(three[..., 3] > 0) == 16                                                      # one ring per pass: 63 passes are needed


def test_the_host_twins_read_and_write_buffers_at_any_address():
    lib = _lib.load()
    src, want = _atlas("special", 17, 9), _dilated("special", 17, 9, 3, True)
    pts, _ = _board()
    for shift in (1, 2, 3, 4, 8):
        raw_src, raw_out = np.zeros(src.nbytes + 16, np.uint8), np.zeros(src.nbytes + 16, np.uint8)
        raw_src[shift:shift + src.nbytes] = src.view(np.uint8).reshape(-1)
        assert lib.brt_host_lightmap_dilate(raw_src.ctypes.data + shift, 17, 9, 3, 1, raw_out.ctypes.data + shift) == 0
        assert_texels_equal(raw_out[shift:shift + src.nbytes].copy().view(F32).reshape(src.shape), want, f"dilate at +{shift}")
        assert not raw_out[:shift].any() and not raw_out[shift + src.nbytes:].any()
        raw_pt, raw_ray = np.zeros(48, np.uint8), np.zeros(48, np.uint8)
        raw_pt[shift:shift + 32] = pts[9:10].view(np.uint8)
        assert lib.brt_host_lightmap_ray(raw_pt.ctypes.data + shift, 65, 64, raw_ray.ctypes.data + shift) == 0
        assert raw_ray[shift:shift + 32].tobytes() == brt.lightmap_ray(pts[9], 65, 64).tobytes() and not raw_ray[shift + 32:].any()
        raw_dir = np.zeros(63 * 12 + 16, np.uint8)
        assert lib.brt_host_lightmap_directions(63, _lib.C.cast(raw_dir.ctypes.data + shift, _lib.C.POINTER(_lib.C.c_float))) == 0
        assert raw_dir[shift:shift + 63 * 12].tobytes() == _dirs(63).tobytes()
        raw_sp = np.zeros(5 * 3 * 32 + 16, np.uint8)
        assert lib.brt_host_lightmap_sphere_points((_lib.C.c_float * 3)(1, 2, 3), 0.5, 9, 1e-3, 5, 3, raw_sp.ctypes.data + shift) == 0
        assert raw_sp[shift:shift + 480].tobytes() == brt.lightmap_sphere_points((1, 2, 3), 0.5, 5, 3, 9, 1e-3).tobytes()


def test_the_sphere_chart():
    pts = brt.lightmap_sphere_points((1.0, -2.0, 3.5), 0.75, 16, 8, seed=0xFFFFFFF0, offset=1e-3)
    pos, nrm = lr.sphere_points64((1.0, -2.0, 3.5), 0.75, 16, 8)
    assert pts.shape == (8, 16) and np.abs(pts["position"] - pos).max() < 5e-7 and np.abs(pts["normal"] - nrm).max() < 1e-7
    assert np.array_equal(pts["seed"].reshape(-1), lr.seeds(0xFFFFFFF0, 128)) and (pts["offset"] == F32(1e-3)).all()
    assert (pts["normal"][0, :, 1] > 0.9).all() and (pts["normal"][7, :, 1] < -0.9).all()                  # row 0 is the cap about +Y
    assert not lr.point_status(pts).any()


def test_every_host_refusal_writes_nothing():
    lib = _lib.load()
    out = np.full(17 * 9 * 4 + 64, 7.0, F32)
    src, pts = _atlas("checker", 17, 9), _board()[0]
    o, s, p = out.ctypes.data, src.ctypes.data, pts.ctypes.data
    fp = out.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
    c3 = (_lib.C.c_float * 3)(1, 2, 3)
    bad3 = (_lib.C.c_float * 3)(1, float("nan"), 3)
    calls = {
        "directions, n 0": lambda: lib.brt_host_lightmap_directions(0, fp),
        "directions, n 65537": lambda: lib.brt_host_lightmap_directions(65537, fp),
        "directions, null": lambda: lib.brt_host_lightmap_directions(4, None),
        "ray, n 0": lambda: lib.brt_host_lightmap_ray(p, 0, 0, o),
        "ray, n 65537": lambda: lib.brt_host_lightmap_ray(p, 65537, 0, o),
        "ray, k = n": lambda: lib.brt_host_lightmap_ray(p, 64, 64, o),
        "ray, null point": lambda: lib.brt_host_lightmap_ray(None, 64, 0, o),
        "ray, null out": lambda: lib.brt_host_lightmap_ray(p, 64, 0, None),
        "ray, overlap": lambda: lib.brt_host_lightmap_ray(o, 64, 0, o + 16),
        "sphere, width 0": lambda: lib.brt_host_lightmap_sphere_points(c3, 1.0, 0, 0.0, 0, 4, o),
        "sphere, height 16385": lambda: lib.brt_host_lightmap_sphere_points(c3, 1.0, 0, 0.0, 4, 16385, o),
        "sphere, null centre": lambda: lib.brt_host_lightmap_sphere_points(None, 1.0, 0, 0.0, 4, 4, o),
        "sphere, null out": lambda: lib.brt_host_lightmap_sphere_points(c3, 1.0, 0, 0.0, 4, 4, None),
        "sphere, a NaN centre": lambda: lib.brt_host_lightmap_sphere_points(bad3, 1.0, 0, 0.0, 4, 4, o),
        "sphere, radius 0": lambda: lib.brt_host_lightmap_sphere_points(c3, 0.0, 0, 0.0, 4, 4, o),
        "sphere, radius INF": lambda: lib.brt_host_lightmap_sphere_points(c3, float("inf"), 0, 0.0, 4, 4, o),
        "sphere, offset < 0": lambda: lib.brt_host_lightmap_sphere_points(c3, 1.0, 0, -1.0, 4, 4, o),
        "sphere, offset NaN": lambda: lib.brt_host_lightmap_sphere_points(c3, 1.0, 0, float("nan"), 4, 4, o),
        "dilate, width 0": lambda: lib.brt_host_lightmap_dilate(s, 0, 9, 1, 0, o),
        "dilate, height 0": lambda: lib.brt_host_lightmap_dilate(s, 17, 0, 1, 0, o),
        "dilate, width 16385": lambda: lib.brt_host_lightmap_dilate(s, 16385, 1, 1, 0, o),
        "dilate, passes 65": lambda: lib.brt_host_lightmap_dilate(s, 17, 9, 65, 0, o),
        "dilate, wrap_u 2": lambda: lib.brt_host_lightmap_dilate(s, 17, 9, 1, 2, o),
        "dilate, null src": lambda: lib.brt_host_lightmap_dilate(None, 17, 9, 1, 0, o),
        "dilate, null out": lambda: lib.brt_host_lightmap_dilate(s, 17, 9, 1, 0, None),
        "dilate, overlap": lambda: lib.brt_host_lightmap_dilate(o, 17, 9, 1, 0, o + 64),
    }
    for what, call in calls.items():
        assert call() == INVALID, what
        assert (out == 7.0).all(), f"{what}: something was written"
        assert lib.brt_last_error(None), what
    with pytest.raises(brt.BrtError):
        brt.lightmap_directions(0)
    assert_texels_equal(brt.lightmap_dilate_host(src, 1, False), _dilated("checker", 17, 9, 1, False))


CONTACT_N, CONTACT_W, CONTACT_H, CONTACT_BOUNCES = 16, 8, 4, 4


@functools.lru_cache(maxsize=None)
def _contact():
    """A unit sphere resting on the ground sphere, both grey, and the 8 x 4 chart of the unit sphere."""
    grey = brt.StandardMaterial(base_color=(0.5, 0.5, 0.5))
    b = make_buffers([((0.0, -1000.0, 0.0), 1000.0, grey), ((0.0, 1.0, 0.0), 1.0, grey)])
    pts = brt.lightmap_sphere_points((0.0, 1.0, 0.0), 1.0, CONTACT_W, CONTACT_H, seed=7, offset=1e-3)
    return b, pts


def _darkens(texels, info):
    """Whether the lowest row is darker and more enclosed than the highest -> (the two mean radiances, the two mean hit shares)."""
    lum = texels[..., :3].astype(np.float64).mean(axis=(1, 2))
    shut = info["hits"].astype(np.float64).mean(axis=1) / CONTACT_N
    return (lum[0], lum[-1]), (shut[0], shut[-1])


def test_the_reference_alone_shows_contact_darkening():
    b, pts = _contact()
    _, cam, _ = brt.cover_camera(16, 16, 1, CONTACT_BOUNCES, brt.Raytracing.Pure, 0.5)
    rays = lr.make_rays(pts, _dirs(CONTACT_N)).reshape(CONTACT_H, CONTACT_W * CONTACT_N)
    rows = [lr.resolve(rr.expected(b.models, b.materials, b.bvh, cam, rays[y], 1, CONTACT_BOUNCES)[0], pts[y], CONTACT_N) for y in (0, CONTACT_H - 1)]
    (top, bottom), (shut_top, shut_bottom) = _darkens(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
    print(f"reference: mean radiance {top:.3f} at the top row, {bottom:.3f} at the bottom; hit share {shut_top:.3f}, {shut_bottom:.3f}")
    assert bottom < 0.5 * top and shut_bottom > shut_top + 0.5                                            # (by a wide margin at this N)


def test_the_stand_alone_twin_under_sanitizers(tmp_path):
    """tests/tools/lightmap_twin_main.hip: the host rule alone in a program of its own, built with the address and undefined-behaviour
    sanitizers and run on the CPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "lightmap_twin_main")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "bevyray_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "tools", "lightmap_twin_main.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _read(d_buf, n_bytes, fill, what):
    import torch
    torch.cuda.synchronize()
    got = d_buf.cpu().numpy()
    assert (got[n_bytes:] == fill).all(), f"{what}: the guard was written"
    return got[:n_bytes].copy()


def _texel_bytes(fmt):
    return 8 if fmt == RGBA16F else 16


def _as_texels(raw, fmt, shape):
    return raw.view(np.float16 if fmt == RGBA16F else F32).reshape(*shape, 4)


def _dilate_device(plugin, src, passes, wrap, fmt=0, stream=None):
    h, w = src.shape[:2]
    n = w * h * _texel_bytes(fmt)
    d_src, d_out = _dev(src), _guarded(n, 16 * w, 0xCD)                                                   # (a guard row)
    plugin.node.lightmap_dilate_device(d_src.data_ptr(), w, h, passes, wrap, d_out.data_ptr(), stream=stream, out_format=fmt)
    return _as_texels(_read(d_out, n, 0xCD, "dilate"), fmt, (h, w))


def _resolve_device(plugin, results, points, n_dirs, fmt=0, info=True):
    n = len(points)
    d_res, d_pts = _dev(results), _dev(points)
    d_out, d_info = _guarded(n * _texel_bytes(fmt), 16, 0xCD), _guarded(n * 8, 16, 0xEE)                  # (a guard texel)
    plugin.node.lightmap_resolve_device(d_res.data_ptr(), d_pts.data_ptr(), n, n_dirs, d_out.data_ptr(), d_info.data_ptr() if info else 0,
                                        out_format=fmt)
    texels = _as_texels(_read(d_out, n * _texel_bytes(fmt), 0xCD, "resolve"), fmt, (n,))
    raw_info = _read(d_info, n * 8 if info else 0, 0xEE, "info")
    return texels, raw_info.view(INFO) if info else None


@pytest.mark.gpu
@pytest.mark.parametrize("n_dirs", [1, 63, 64, 65, 256])
def test_generated_rays_are_the_host_twin_on_the_board(plugin, n_dirs):
    pts, _ = _board()
    n = len(pts) * n_dirs
    d_pts, d_rays = _dev(pts), _guarded(n * 32, 32, 0xAB)                                                 # (a guard record)
    plugin.node.lightmap_rays_device(d_pts.data_ptr(), len(pts), n_dirs, d_rays.data_ptr())
    got = _read(d_rays, n * 32, 0xAB, "rays").view(brt.RADIANCE_RAY_DTYPE)
    assert np.array_equal(got.view(np.uint32), _twin_rays(pts, n_dirs).view(np.uint32))
    assert np.array_equal(got.view(np.uint32), lr.make_rays(pts, _dirs(n_dirs)).view(np.uint32))


def _synthetic_results(n_points, n_dirs, seed):
    rng = np.random.default_rng([72, n_points, n_dirs, seed])
    n = n_points * n_dirs
    res = np.zeros(n, brt.RADIANCE_DTYPE)
    res["t"] = rng.uniform(0, 50, n)
    res["rgb"] = rng.uniform(0, 2, size=(n, 3)).astype(F32)
    res["status"] = rng.choice([0, 1, 3], size=n)
    res["sphere"], res["material"], res["user"] = 0xFFFFFFFF, 7, np.tile(np.arange(n_dirs), n_points)
    by = res.reshape(n_points, n_dirs)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 3e38, 1e-30, -0.0, 1e-42)):
        by["rgb"][(2 + k) % n_points, (5 * k) % n_dirs, k % 3] = v
    pts = np.zeros(n_points, POINT)
    pts["normal"] = rng.normal(size=(n_points, 3)).astype(F32)
    # point 1 refused as INVALID, point 3 as OUT_OF_REACH (every entry, as the radiance kernels refuse a point), point 4 EMPTY, point 5
    # EMPTY with entries that say otherwise, point 6 all -0.0
    for p, st in ((1, INVALID_BIT), (3, OUT_OF_REACH)):
        by["status"][p] = st
    pts["normal"][4] = 0
    by["status"][4] = INVALID_BIT
    pts["normal"][5] = (-0.0, 0.0, -0.0)
    by["rgb"][6] = -0.0
    return res, pts


@pytest.mark.gpu
@pytest.mark.parametrize("n_dirs", [1, 63, 64, 65, 200])
def test_the_resolve_kernel_on_synthetic_results(plugin, n_dirs):
    n_points = 9                                                                                          # (more than the 4 waves of a block)
    res, pts = _synthetic_results(n_points, n_dirs, 0)
    want, want_info = lr.resolve(res, pts, n_dirs)
    assert list(want_info["status"][[0, 1, 3, 4, 5]]) == [0, INVALID_BIT, OUT_OF_REACH, EMPTY, EMPTY]
    assert not want[[1, 3, 4, 5]].any() and not want_info["hits"][[1, 3, 4, 5]].any() and (want[[0, 2, 6, 7, 8], 3] == 1).all()
    assert np.isnan(want).any() or n_dirs == 1
    assert not want[6, :3].any() and not np.signbit(want[6, :3]).any()                                    # (-0.0 squared is +0.0)
    for fmt in (0, RGBA16F):
        for info in (True, False):
            got, got_info = _resolve_device(plugin, res, pts, n_dirs, fmt, info)
            with np.errstate(over="ignore"):
                assert_texels_equal(got, want.astype(np.float16) if fmt else want, f"N {n_dirs} format {fmt} info {info}")
            if info:
                assert got_info.tobytes() == want_info.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES + [(16384, 1), (1, 16384)])
def test_the_dilate_kernel_is_the_host_twin_and_the_restatement(plugin, size):
    w, h = size
    big = w * h == 16384
    for kind in (("checker", "special") if big else ATLASES):
        src = _atlas(kind, w, h)
        for passes in ((0, 3) if big else PASSES):
            for wrap in (False, True):
                twin = brt.lightmap_dilate_host(src, passes, wrap)
                what = f"{kind} {size} passes {passes} wrap {wrap}"
                if not big:
                    assert_texels_equal(twin, _dilated(kind, w, h, passes, wrap), what + ", twin")
                assert_texels_equal(_dilate_device(plugin, src, passes, wrap), twin, what)
                with np.errstate(over="ignore"):
                    assert_texels_equal(_dilate_device(plugin, src, passes, wrap, RGBA16F), twin.astype(np.float16), what + ", RGBA16F")


BW, BH, BN, BPASSES = 16, 8, 64, 2


@functools.lru_cache(maxsize=None)
def _bake_points():
    """The 16 x 8 chart of the small sphere of the cover scene nearest (0, 0.2, 0), offset 1e-3 radii, rows 2 and 5 EMPTY."""
    m = _cover().models
    small = np.flatnonzero(m["radius"] == F32(0.2))
    i = small[np.argmin(np.abs(m["position"][small].astype(np.float64) - (0.0, 0.2, 0.0)).sum(axis=1))]
    pts = brt.lightmap_sphere_points(m["position"][i], 0.2, BW, BH, seed=0xFFFFFF80, offset=1e-3 * 0.2).copy()
    pts["normal"][[2, 5]] = 0
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _bake_rays():
    r = _twin_rays(_bake_points(), BN)
    r.setflags(write=False)
    return r


def _steps(plugin, points, n_dirs, bounces, passes, wrap, fmt=0, **knobs):
    """The bake through the step exports: rays -> brt_radiance_rays_device -> resolve -> dilate.  -> (texels, info, the radiance
    results, the radiance call's stats)."""
    h, w = points.shape
    n = w * h
    d_pts, d_rays, d_res = _dev(points), _guarded(n * n_dirs * 32, 32, 0xAB), _guarded(n * n_dirs * 32, 32, 0xAB)
    d_img, d_info, d_out = _guarded(n * 16, 16, 0xCD), _guarded(n * 8, 16, 0xEE), _guarded(n * _texel_bytes(fmt), 16, 0xCD)
    plugin.node.lightmap_rays_device(d_pts.data_ptr(), n, n_dirs, d_rays.data_ptr())
    with plugin.tuning(**knobs):
        rad = dict(plugin.node.radiance_rays((d_rays.data_ptr(), n * n_dirs, d_res.data_ptr()), 1, bounces, device=True))
    plugin.node.lightmap_resolve_device(d_res.data_ptr(), d_pts.data_ptr(), n, n_dirs, d_img.data_ptr(), d_info.data_ptr())
    plugin.node.lightmap_dilate_device(d_img.data_ptr(), w, h, passes, wrap, d_out.data_ptr(), out_format=fmt)
    texels = _as_texels(_read(d_out, n * _texel_bytes(fmt), 0xCD, "steps"), fmt, (h, w))
    info = _read(d_info, n * 8, 0xEE, "steps, info").view(INFO).reshape(h, w)
    results = _read(d_res, n * n_dirs * 32, 0xAB, "steps, results").view(brt.RADIANCE_DTYPE)
    rays = _read(d_rays, n * n_dirs * 32, 0xAB, "steps, rays").view(brt.RADIANCE_RAY_DTYPE)
    return texels, info, results, rad, rays


def _bake_device(plugin, points, n_dirs, bounces, passes, wrap, fmt=0, stream=None, info=True, origin_bound=0.0, **knobs):
    h, w = points.shape
    n = w * h
    d_pts, d_out, d_info = _dev(points), _guarded(n * _texel_bytes(fmt), 16 * w, 0xCD), _guarded(n * 8, 16, 0xEE)
    with plugin.tuning(**knobs):
        st = dict(plugin.node.bake_lightmap((d_pts.data_ptr(), w, h, d_out.data_ptr(), d_info.data_ptr() if info else 0), n_dirs, bounces, passes,
                                            wrap, origin_bound, device=True, stream=stream, out_format=fmt))
    texels = _as_texels(_read(d_out, n * _texel_bytes(fmt), 0xCD, "bake"), fmt, (h, w))
    raw = _read(d_info, n * 8 if info else 0, 0xEE, "bake, info")
    return texels, (raw.view(INFO).reshape(h, w) if info else None), st


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [0, 8])
@pytest.mark.parametrize("tree", ["caller", "callee"])
def test_a_bake_is_the_radiance_call_the_restated_resolve_and_dilate_and_its_own_steps(plugin, tree, bounces):
    _upload_cover(plugin, tree)
    pts = _bake_points()
    n, entries = BW * BH, BW * BH * BN
    want, want_info, results, rad, rays = _steps(plugin, pts, BN, bounces, BPASSES, True)
    # the generated list is the twin's, and the results are the radiance call's over the twin's entries
    assert np.array_equal(rays.view(np.uint32), _bake_rays().view(np.uint32))
    d_rays, d_res = _dev(_bake_rays()), _guarded(entries * 32, 32, 0xAB)
    rad2 = dict(plugin.node.radiance_rays((d_rays.data_ptr(), entries, d_res.data_ptr()), 1, bounces, device=True))
    twin_results = _read(d_res, entries * 32, 0xAB, "the twin's entries").view(brt.RADIANCE_DTYPE)
    rr.assert_equal(results, twin_results, "the generated list")
    assert rad2 == rad
    # ... resolved and dilated by the restatement
    img, info = lr.resolve(twin_results, pts.reshape(-1), BN)
    empty = np.zeros((BH, BW), bool)
    empty[[2, 5]] = True
    hit = (twin_results["status"] & 1) != 0
    traced = entries - 2 * BW * BN
    assert (info["status"].reshape(BH, BW) == np.where(empty, EMPTY, 0)).all() and not img.reshape(BH, BW, 4)[empty].any()
    assert (img.reshape(BH, BW, 4)[~empty, 3] == 1).all() and BN < hit.sum() < traced - BN                 # (the chart sees spheres and sky)
    assert len(np.unique(img[:, 0])) > n // 2
    assert (rad["walks"] >= traced) and (rad["hits"], rad["refused"]) == (int(hit.sum()), entries - traced)
    if bounces == 0:
        assert rad["walks"] == traced                                                                    # one walk per entry that is not refused
    assert_texels_equal(want, lr.dilate(img.reshape(BH, BW, 4), BPASSES, True), "the steps")
    assert want_info.tobytes() == info.reshape(BH, BW).tobytes()
    assert (want[[2, 5], :, 3] == 0.5).all() and want[[2, 5], :, :3].any()                                # the EMPTY rows are filled from their neighbours
    seen = {}
    for form in (PLAIN, STREAM):
        for chunks, knobs in ((1, {}), (7, {"BRT_PROBE_CHUNK_RAYS": 19 * BN}), (n, {"BRT_PROBE_CHUNK_RAYS": 1})):
            what = f"{tree} bounces {bounces} form {form} chunks {chunks}"
            got, got_info, st = _bake_device(plugin, pts, BN, bounces, BPASSES, True, BRT_RADIANCE_FORM=form, **knobs)
            assert_texels_equal(got, want, what)
            assert got_info.tobytes() == want_info.tobytes(), what
            assert (st["walks"], st["hits"], st["refused"], st["chunks"], st["form"]) == (rad["walks"], rad["hits"], rad["refused"], chunks, form - 1), (what, st, rad)
            with plugin.tuning(BRT_RADIANCE_FORM=form, **knobs):
                host, host_info = plugin.node.bake_lightmap(pts, BN, bounces, BPASSES, True)
            assert_texels_equal(host, want, what + ", host")
            assert host_info.tobytes() == want_info.tobytes() and plugin.node.last_probe_stats == st, what
            seen[form, chunks] = got.tobytes()
    assert len(set(seen.values())) == 1
    # the other output format, no info buffer, no passes (the resolve then writes the target itself), one pass, no wrap
    seven = {"BRT_PROBE_CHUNK_RAYS": 19 * BN}
    half, _, _ = _bake_device(plugin, pts, BN, bounces, BPASSES, True, RGBA16F, info=False, **seven)
    assert_texels_equal(half, want.astype(np.float16), "RGBA16F")
    with plugin.tuning(**seven):
        host16, none = plugin.node.bake_lightmap(pts, BN, bounces, BPASSES, True, out_format=RGBA16F, info=False)
    assert none is None
    assert_texels_equal(host16, want.astype(np.float16), "host, RGBA16F")
    for fmt in (0, RGBA16F):
        raw, raw_info, _ = _bake_device(plugin, pts, BN, bounces, 0, False, fmt, **seven)
        assert_texels_equal(raw, img.reshape(BH, BW, 4).astype(np.float16 if fmt else F32), f"no passes, format {fmt}")
        assert raw_info.tobytes() == want_info.tobytes()
    one, _, _ = _bake_device(plugin, pts, BN, bounces, 1, False)
    assert_texels_equal(one, lr.dilate(img.reshape(BH, BW, 4), 1, False), "one pass, no wrap")
    assert_texels_equal(plugin.node.bake_lightmap(pts, BN, bounces, 0)[0], img.reshape(BH, BW, 4), "host, no passes")


@pytest.mark.gpu
def test_an_empty_sky(plugin):
    plugin.node.write_buffers(make_buffers([((300.0, 400.0, 500.0), 0.01, brt.StandardMaterial())]))
    pts = _points([((0.5, 1.0, -2.0), 9, (0.0, 1.0, 0.0), 0.0), ((0.5, 1.0, -2.0), 10, (0.0, 3.0, 0.0), 0.25), ((0.5, 1.0, -2.0), 11, (0.0, -1.0, 0.0), 0.0)]).reshape(1, 3)
    got, info, st = _bake_device(plugin, pts, SKY_N, 8, 0, False)
    assert (st["hits"], st["refused"], st["walks"]) == (0, 0, 3 * SKY_N) and not info["hits"].any() and not info["status"].any()
    assert (got[0, :, 3] == 1).all()
    up = lr.SKY_A + (2.0 / 3.0) * lr.SKY_B                      # the cosine-weighted mean of A + B d_y about n is A + (2/3) B n_y
    down = lr.SKY_A - (2.0 / 3.0) * lr.SKY_B
    err = max(np.abs(got[0, 0, :3] - up).max(), np.abs(got[0, 1, :3] - up).max(), np.abs(got[0, 2, :3] - down).max())
    print(f"empty sky, {SKY_N} directions: largest |rgb - closed form| {err:.3e}")
    assert err <= SKY_QUADRATURE + 1e-5
    # and bitwise the restated resolve of the closed-form miss colour of every entry
    rays = lr.make_rays(pts, _dirs(SKY_N))
    res = np.zeros(len(rays), brt.RADIANCE_DTYPE)
    res["rgb"] = rr.sky_rgb(rays["direction"])
    assert_texels_equal(got.reshape(3, 4), lr.resolve(res, pts.reshape(-1), SKY_N)[0], "the restated resolve of the sky")


@pytest.mark.gpu
def test_contact_darkening(plugin):
    b, pts = _contact()
    plugin.node.write_buffers(b)
    got, info, st = _bake_device(plugin, pts, CONTACT_N, CONTACT_BOUNCES, 0, False)
    assert st["refused"] == 0 and not info["status"].any() and (got[..., 3] == 1).all()
    (top, bottom), (shut_top, shut_bottom) = _darkens(got, info)
    print(f"bake: mean radiance {top:.3f} at the top row, {bottom:.3f} at the bottom; hit share {shut_top:.3f}, {shut_bottom:.3f}")
    assert bottom < top and shut_bottom > shut_top
    # ... and it is the reference's bake of those two rows, bitwise
    _, cam, _ = brt.cover_camera(16, 16, 1, CONTACT_BOUNCES, brt.Raytracing.Pure, 0.5)
    rays = lr.make_rays(pts, _dirs(CONTACT_N)).reshape(CONTACT_H, CONTACT_W * CONTACT_N)
    for y in (0, CONTACT_H - 1):
        want, want_info = lr.resolve(rr.expected(b.models, b.materials, b.bvh, cam, rays[y], 1, CONTACT_BOUNCES)[0], pts[y], CONTACT_N)
        assert_texels_equal(got[y], want, f"row {y}")
        assert info[y].tobytes() == want_info.tobytes()


@pytest.mark.gpu
def test_a_point_beyond_the_trees_reach(plugin):
    _upload_cover(plugin, "callee")
    bound = plugin.node.query_origin_bound()
    assert 40.0 <= bound < np.inf
    far = (13.0 * 60.0, 2.0 * 60.0, 3.0 * 60.0)
    pts = np.concatenate([_bake_points()[0, :2], _points([(far, 9, (0.0, -1.0, 0.0), 0.0), ((np.nan, 0.0, 0.0), 3, (0.0, 1.0, 0.0), 0.0)])]).reshape(1, 4)
    near_alone, near_info, _ = _bake_device(plugin, pts[:, :2], BN, 4, 0, False)
    for device in (True, False):
        if device:
            got, info, st = _bake_device(plugin, pts, BN, 4, 0, False)
        else:
            got, info = plugin.node.bake_lightmap(pts, BN, 4, 0)
            st = plugin.node.last_probe_stats
        assert list(info["status"][0]) == [0, 0, OUT_OF_REACH, INVALID_BIT] and st["refused"] == 2 * BN and st["tree_rebuilt"] == 0
        assert not got[0, 2:].any() and not info["hits"][0, 2:].any()
        assert_texels_equal(got[:, :2], near_alone, "neighbours of refused points")
    l1 = l1_norm(far)
    got, info, st = _bake_device(plugin, pts, BN, 4, 0, False, origin_bound=l1 + 1.0)
    assert list(info["status"][0]) == [0, 0, 0, INVALID_BIT] and st["tree_rebuilt"] == 1 and plugin.node.query_origin_bound() >= l1
    assert got[0, 2, 3] == 1 and got[0, 2, :3].all() and st["refused"] == BN
    # the far point looks down at the scene from above: mostly ground, by the radiance call over its entries on the same tree
    d_rays, d_res = _dev(_twin_rays(pts[0, 2:3], BN)), _guarded(BN * 32, 32, 0xAB)
    plugin.node.radiance_rays((d_rays.data_ptr(), BN, d_res.data_ptr()), 1, 4, device=True)
    res = _read(d_res, BN * 32, 0xAB, "far").view(brt.RADIANCE_DTYPE)
    assert_texels_equal(got[0, 2:3], lr.resolve(res, pts[0, 2:3], BN)[0], "the far point")
    _, _, st = _bake_device(plugin, pts, BN, 4, 0, False, origin_bound=l1 + 1.0)
    assert st["tree_rebuilt"] == 0
    plugin.node.write_buffers(_cover())


@pytest.mark.gpu
def test_a_scene_with_32_bit_descriptors(plugin):
    s = big_scene(16383, 11)
    b = brt.Buffers(s.models, s.materials, brt.build_bvh(s.models))
    lvl, cam, win = big_view(96, 54)
    plugin.node.run(lvl, cam, win, 96, 54, buffers=b)
    assert plugin.node.last_stats["scene_in_lds"] == 0
    i = int(np.argmin(np.abs(b.models["position"].astype(np.float64) - b.models["position"].astype(np.float64).mean(axis=0)).sum(axis=1)))
    radius = float(b.models["radius"][i])
    pts = brt.lightmap_sphere_points(b.models["position"][i], radius, 8, 6, seed=77, offset=1e-3 * radius)
    want, want_info, _, rad, _ = _steps(plugin, pts, BN, 4, 1, True)
    assert rad["hits"] > 50 and rad["form"] == 0
    got, info, st = _bake_device(plugin, pts, BN, 4, 1, True, BRT_PROBE_CHUNK_RAYS=10 * BN)
    assert_texels_equal(got, want, "32-bit descriptors")
    assert info.tobytes() == want_info.tobytes()
    assert st["form"] == 0 and st["chunks"] == 5 and (st["walks"], st["hits"]) == (rad["walks"], rad["hits"])     # (no LDS form: the plain kernel)
    with plugin.tuning(BRT_RADIANCE_FORM=STREAM):
        assert_texels_equal(plugin.node.bake_lightmap(pts, BN, 4, 1, True)[0], want, "streaming")
        assert plugin.node.last_probe_stats["form"] == 1


@pytest.mark.gpu
def test_streams_uploads_frames_and_refusals(plugin):
    import torch
    b = _cover()
    w, h = 160, 90
    lvl, cam, win = brt.cover_camera(w, h, 2, 4, brt.Raytracing.Pure, 0.5)
    before = plugin.node.run(lvl, cam, win, w, h, buffers=b, flags=brt.FLAG_COUNTERS).copy()
    stats_before = dict(plugin.node.last_stats)
    pts = _bake_points()
    n = BW * BH
    args = (pts, BN, 4, 0, False)
    serial, serial_info, _ = _bake_device(plugin, *args)
    dilated = lr.dilate(serial, 3, True)
    # a bake on one caller stream, the dilation of its image on another: the same bytes
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_pts = _dev(pts)
    d_img, d_info, d_dil = (torch.zeros(n * k, dtype=torch.uint8, device="cuda") for k in (16, 8, 16))
    torch.cuda.synchronize()

    def on_two_streams(between=None):
        for t in (d_img, d_info, d_dil):
            t.zero_()
        torch.cuda.synchronize()
        st = plugin.node.bake_lightmap((d_pts.data_ptr(), BW, BH, d_img.data_ptr(), d_info.data_ptr()), BN, 4, 0, False, device=True, stream=s1.cuda_stream)
        assert (st["walks"], st["hits"], st["refused"], st["chunks"]) == (0, 0, 0, 1)
        if between:
            between()
        plugin.node.lightmap_dilate_device(d_img.data_ptr(), BW, BH, 3, True, d_dil.data_ptr(), stream=s2.cuda_stream)
        torch.cuda.synchronize()
        assert_texels_equal(d_img.cpu().numpy().view(F32).reshape(BH, BW, 4), serial, "two streams")
        assert d_info.cpu().numpy().tobytes() == serial_info.tobytes()
        assert_texels_equal(d_dil.cpu().numpy().view(F32).reshape(BH, BW, 4), dilated, "two streams, the dilation")

    on_two_streams()
    # an upload between the bake and the dilation waits for the bake and changes nothing in either
    moved = b.models.copy()
    moved["position"][np.flatnonzero(moved["radius"] == 1.0)] += np.array([0.0, 0.6, 0.0], F32)
    on_two_streams(lambda: plugin.node.write_buffers(brt.Buffers(moved, b.materials, brt.build_bvh(moved))))
    assert _bake_device(plugin, *args)[0].tobytes() != serial.tobytes()                                   # (the new scene bakes another chart)
    plugin.node.write_buffers(b)

    # every refusal writes nothing and is followed by a correct call
    lib, ctx = plugin._lib, plugin._ctx
    d_buf = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")
    A = d_buf.data_ptr()
    B, I, T = A + (1 << 19), A + (1 << 18), A + (3 << 18)
    host_pts = np.ascontiguousarray(pts)
    host_out, host_info = np.full((BH, BW, 4), 3.0, F32), np.full(n * 2, 3, np.uint32)
    P, H, HI = host_pts.ctypes.data, host_out.ctypes.data, host_info.ctypes.data

    def refused(code, call, what):
        assert call() == code, what
        torch.cuda.synchronize()
        assert bool((d_buf == 0x5A).all()) and (host_out == 3.0).all() and (host_info == 3).all(), f"{what}: something was written"
        assert_texels_equal(_bake_device(plugin, *args)[0], serial, f"after {what}")

    def bake(points=A, width=BW, height=BH, n_dirs=BN, bounces=4, passes=1, wrap=0, bound=0.0, out=B, info=I, flags=0):
        return lambda: lib.brt_bake_lightmap_device(ctx, points, width, height, n_dirs, bounces, passes, wrap, bound, out, info, None, flags, None)

    def host(points=P, width=BW, height=BH, n_dirs=BN, bounces=4, passes=1, wrap=0, bound=0.0, out=H, info=HI, flags=0):
        return lambda: lib.brt_bake_lightmap(ctx, points, width, height, n_dirs, bounces, passes, wrap, bound, out, info, flags, None)

    for kind, call in (("device", bake), ("host", host)):
        refused(INVALID, call(points=None), f"{kind}, null points")
        refused(INVALID, call(out=None), f"{kind}, null out")
        refused(INVALID, call(width=0), f"{kind}, width 0")
        refused(INVALID, call(height=0), f"{kind}, height 0")
        refused(INVALID, call(width=16385), f"{kind}, width 16385")
        refused(INVALID, call(height=16385), f"{kind}, height 16385")
        refused(INVALID, call(n_dirs=0), f"{kind}, n_dirs 0")
        refused(INVALID, call(n_dirs=65537), f"{kind}, n_dirs 65537")
        refused(INVALID, call(bounces=65536), f"{kind}, bounces 65536")
        refused(INVALID, call(passes=65), f"{kind}, passes 65")
        refused(INVALID, call(wrap=2), f"{kind}, wrap_u 2")
        refused(INVALID, call(bound=float("nan")), f"{kind}, origin_bound NaN")
        refused(INVALID, call(bound=-1.0), f"{kind}, origin_bound < 0")
        refused(INVALID, call(bound=float("inf")), f"{kind}, origin_bound INF")
        refused(INVALID, call(flags=brt.FLAG_DENOISE), f"{kind}, an unknown flag")
        refused(INVALID, call(flags=brt.FLAG_OUT_RGBA8_UNORM), f"{kind}, another output format")
    refused(INVALID, bake(out=A + 64), "device, out over points")
    refused(INVALID, bake(info=A + 64), "device, info over points")
    refused(INVALID, bake(info=B + 64), "device, info over out")
    refused(INVALID, bake(out=B + 8), "device, out not 16-byte aligned")
    refused(INVALID, bake(points=A + 4), "device, points not 16-byte aligned")
    refused(INVALID, host(out=P + 64), "host, out over points")
    refused(INVALID, host(info=H + 64), "host, info over out")
    refused(INVALID, host(flags=brt.FLAG_CALLER_STREAM), "host, the stream flag")

    def rays(points=A, n_points=n, n_dirs=BN, out=B, flags=0):
        return lambda: lib.brt_lightmap_rays_device(ctx, points, n_points, n_dirs, out, None, flags)

    refused(INVALID, rays(points=None), "rays, null points")
    refused(INVALID, rays(out=None), "rays, null rays")
    refused(INVALID, rays(n_dirs=0), "rays, n_dirs 0")
    refused(INVALID, rays(n_dirs=65537), "rays, n_dirs 65537")
    refused(INVALID, rays(n_points=1 << 16, n_dirs=1 << 15), "rays, too many entries")
    refused(INVALID, rays(out=A + 64), "rays, overlap")
    refused(INVALID, rays(out=B + 8), "rays, not 16-byte aligned")
    refused(INVALID, rays(flags=RGBA16F), "rays, an unknown flag")

    def resolve(results=A, points=T, n_points=n, n_dirs=4, out=B, info=I, flags=0):
        return lambda: lib.brt_lightmap_resolve_device(ctx, results, points, n_points, n_dirs, out, info, None, flags)

    refused(INVALID, resolve(results=None), "resolve, null results")
    refused(INVALID, resolve(points=None), "resolve, null points")
    refused(INVALID, resolve(out=None), "resolve, null out")
    refused(INVALID, resolve(n_dirs=0), "resolve, n_dirs 0")
    refused(INVALID, resolve(n_points=1 << 16, n_dirs=1 << 15), "resolve, too many entries")
    refused(INVALID, resolve(out=A + 64), "resolve, out over results")
    refused(INVALID, resolve(out=T + 64), "resolve, out over points")
    refused(INVALID, resolve(info=B + 64), "resolve, info over out")
    refused(INVALID, resolve(info=A + 64), "resolve, info over results")
    refused(INVALID, resolve(info=I + 8), "resolve, info not 16-byte aligned")
    refused(INVALID, resolve(flags=brt.FLAG_OUT_RGBA8_UNORM_SRGB), "resolve, an unknown flag")

    def dilate(src=A, width=BW, height=BH, passes=1, wrap=0, out=B, flags=0):
        return lambda: lib.brt_lightmap_dilate_device(ctx, src, width, height, passes, wrap, out, None, flags)

    refused(INVALID, dilate(src=None), "dilate, null src")
    refused(INVALID, dilate(out=None), "dilate, null out")
    refused(INVALID, dilate(width=0), "dilate, width 0")
    refused(INVALID, dilate(height=16385), "dilate, height 16385")
    refused(INVALID, dilate(passes=65), "dilate, passes 65")
    refused(INVALID, dilate(wrap=2), "dilate, wrap_u 2")
    refused(INVALID, dilate(out=A + 64), "dilate, overlap")
    refused(INVALID, dilate(src=A + 8), "dilate, not 16-byte aligned")
    refused(INVALID, dilate(flags=brt.FLAG_TEMPORAL), "dilate, an unknown flag")
    # an empty list is no error for the two list steps
    assert lib.brt_lightmap_rays_device(ctx, None, 0, BN, None, None, 0) == 0
    assert lib.brt_lightmap_resolve_device(ctx, None, None, 0, BN, None, None, None, 0) == 0
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        assert bake()() == UNSUPPORTED and host()() == UNSUPPORTED
    finally:
        plugin.set_policy(0)
    torch.cuda.synchronize()
    assert bool((d_buf == 0x5A).all()) and (host_out == 3.0).all() and (host_info == 3).all(), "a bake under a policy wrote something"
    assert_texels_equal(_bake_device(plugin, *args)[0], serial, "after the bakes under a policy")
    with brt.RaytracePlugin([0]) as empty:
        for call in (lambda: empty.node.bake_lightmap(pts, BN, 4), lambda: empty.node.bake_lightmap((A, BW, BH, B, I), BN, 4, device=True)):
            with pytest.raises(brt.BrtError) as e:
                call()
            assert e.value.code == NO_SCENE
        d_s, d_o = _dev(serial), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        empty.node.lightmap_dilate_device(d_s.data_ptr(), BW, BH, 3, True, d_o.data_ptr())              # the steps need no scene
        assert_texels_equal(d_o.cpu().numpy().view(F32).reshape(BH, BW, 4), dilated, "without a scene")
        empty.node.write_buffers(b)
        assert_texels_equal(empty.node.bake_lightmap(pts, BN, 4)[0], serial, "another context")
    assert bool((d_buf == 0x5A).all())

    # a plain frame after all of it is the frame before
    after = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_COUNTERS)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    for k in ("rays", "node_pops", "interior_visits", "sphere_tests", "hits", "kernel_variant", "n_workgroups", "scene_in_lds"):
        assert plugin.node.last_stats[k] == stats_before[k], k
