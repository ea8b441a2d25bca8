"""Reflection probes (brt_bake_envmap*, brt_envmap_*_device, brt_host_envmap_*; DESIGN.md "Reflection probes").  CPU: the exports, the
texel directions, the tap tables and the host twins of the box level and the filter rule against the restatement (tests/envmap_ref.py)
on synthetic cubes of every category, every refusal, the f32 rule against float64, the closed-form sky, a stand-alone sanitizer
program.  GPU: the four kernels bitwise against the host twins and the restatement; the bake against brt_radiance_rays_device plus the
restated resolve and against its own steps on both trees, both entry points, both radiance forms, two chunkings and both output
formats; an empty sky; 32-bit descriptors; streams, uploads, frames and refusals."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import bevyray_amd as brt
import envmap_ref as er
import radiance_ref as rr
from bevyray_amd import _lib
from helpers import big_scene, big_view, cover as _cover, dev as _dev, guarded as _guarded, make_buffers, upload_cover as _upload_cover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("brt_host_envmap_directions", "brt_host_envmap_taps", "brt_host_envmap_downsample", "brt_host_envmap_filter",
           "brt_envmap_rays_device", "brt_envmap_resolve_device", "brt_envmap_downsample_device", "brt_envmap_filter_device",
           "brt_bake_envmap_device", "brt_bake_envmap")
F32 = np.float32
GGX, COSINE = brt.ENVMAP_TAPS_GGX, brt.ENVMAP_TAPS_COSINE
INVALID, UNSUPPORTED, NO_SCENE = -1, -8, -7
PAIRS = [(1, 1), (2, 1), (3, 3), (8, 4), (17, 5), (16, 16)]          # (src_size, dst_size)
CUBES = ("constant", "lit", "gradient", "special")
TABLES = ("one", "ggx25_63", "ggx25_64", "ggx25_65", "ggx100_64", "cosine_256", "zero_64", "nanw_64")
CONSTANT = (0.25, 0.5, 2.0, 1.0)
# |f32 rule - float64 rule| relative to max(1, |ref|), the largest over the finite cubes x PAIRS x the tables of positive weights
# (test_the_f32_rule_against_float64 prints each and holds the measurement to this figure; DESIGN.md section 21 records it); tests
# that compare across roundings allow four times as much
F32_VS_F64 = 1.6e-6
ACROSS_ROUNDINGS = 4 * F32_VS_F64
# |cosine filter, 256 taps, 16 x 16 sky cube - (A + (2/3) B n_y)|: the largest the f32 restatement shows
# (test_the_cosine_map_of_the_analytic_sky prints it), and the bound: four times that
SKY_COSINE_ERROR = 4.6e-4
SKY_COSINE_BOUND = 4 * SKY_COSINE_ERROR
SKY_A, SKY_B = np.array([0.75, 0.85, 1.0]), np.array([-0.25, -0.15, 0.0])        # the linear sky: A + B d_y


@functools.lru_cache(maxsize=None)
def _table(name):
    if name == "one":
        t = brt.envmap_taps(GGX, 0.5, 1)
    elif name.startswith("ggx25"):
        t = brt.envmap_taps(GGX, 0.25, int(name.split("_")[1]))
    elif name == "ggx100_64":
        t = brt.envmap_taps(GGX, 1.0, 64)
    elif name == "cosine_256":
        t = brt.envmap_taps(COSINE, 0.0, 256)
    elif name == "zero_64":
        t = brt.envmap_taps(GGX, 0.25, 64)
        t[:, 3] = 0.0
        t[::2, 3] = -0.0
    else:
        t = brt.envmap_taps(GGX, 0.25, 64)
        t[17, 3] = np.nan
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _cube(kind, size):
    rng = np.random.default_rng([61, size, CUBES.index(kind)])
    d = er.directions(size)
    if kind == "constant":
        c = np.broadcast_to(np.array(CONSTANT, F32), (6, size, size, 4)).copy()
    elif kind == "lit":
        c = np.zeros((6, size, size, 4), F32)
        for face in range(6):
            c[face, rng.integers(0, size), rng.integers(0, size)] = (1.0 + face, 2.0, 0.5, 1.0)
    elif kind == "gradient":
        c = np.concatenate([F32(0.5) + F32(0.5) * d, (np.arange(6, dtype=F32) / F32(5))[:, None, None, None] * np.ones((6, size, size, 1), F32)], axis=3)
    else:
        c = rng.uniform(0, 4, size=(6, size, size, 4)).astype(F32)
        values = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-42, -1e-42, -0.0]
        flat = c.reshape(-1)
        where = rng.permutation(flat.size)[:max(2, min(len(values), flat.size // 8))]
        for k, i in enumerate(where):
            flat[i] = F32(values[(k + size) % len(values)])
    c = np.ascontiguousarray(c, F32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _want(kind, src, dst, table):
    """The restatement's filter of a fixture, computed once, with what it reached."""
    info = {}
    out = er.filter_cube(_cube(kind, src), _table(table), dst, info=info)
    out.setflags(write=False)
    return out, info


def assert_texels_equal(got, want, what=""):
    """Bitwise, but a NaN for a NaN whatever its sign and payload (the host's and the device's default NaNs differ)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaNs at other places"
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    same = got.view(bits) == want.view(bits)
    assert (same | gn).all(), f"{what}: {np.count_nonzero(~(same | gn))} values differ, first at {np.argwhere(~(same | gn))[0]}"


def _rel(a, b):
    return np.abs(a.astype(np.float64) - b) / np.maximum(1.0, np.abs(b))


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_in_header_ctypes_rust_and_library():
    header = open(os.path.join(ROOT, "include", "bevyray_amd.h")).read()
    rust = open(os.path.join(ROOT, "integration", "bevyray_amd_sys", "src", "lib.rs")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    for name in EXPORTS:
        assert f"int32_t {name}(" in header and name in _lib.EXPORTS and f"pub fn {name}(" in rust and f" T {name}\n" in out, name
    for const in ("BRT_ENVMAP_TAPS_GGX", "BRT_ENVMAP_TAPS_COSINE"):
        assert f"#define {const} " in header and f"pub const {const}: u32" in rust
    assert (GGX, COSINE) == (0, 1)
    assert brt.ENVMAP_TEXEL_DTYPE.itemsize == 16 and brt.ENVMAP_TEXEL16_DTYPE.itemsize == 8 and brt.ENVMAP_TAP_DTYPE.itemsize == 16
    assert brt.envmap_level_offsets(8, 4) == er.level_offsets(8, 4) == [0, 384, 480, 504, 510]
    assert brt.envmap_level_offsets(1024, 11)[-1] == 6 * sum(4 ** k for k in range(11))
    assert _lib.load().brt_abi_version() == 6


@pytest.mark.parametrize("size", [1, 2, 3, 8, 17, 1024])
def test_the_directions_against_the_restatement(size):
    got = brt.envmap_directions(size)
    want = er.directions(size)
    assert got.shape == (6, size, size, 3) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # unit length to within the f32 rounding the restatement shows against its float64 form
    d64 = er.directions(size, np.float64)
    rounding = np.abs(want.astype(np.float64) - d64).max()                             # (0 at size 1: the axes themselves)
    length = np.sqrt((got.astype(np.float64) ** 2).sum(axis=3))
    assert rounding <= 4 * 2.0 ** -24 and np.abs(length - 1.0).max() <= 2 * rounding      # (|d| - 1 <= the error vector's norm)
    if size % 2 == 1:                                                                   # the centre texel of a face is its axis
        axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
        assert np.array_equal(got[:, size // 2, size // 2], axes)
    # every direction lies on its own face under the filter's major-axis rule
    a = np.abs(got)
    major = np.where((a[..., 0] >= a[..., 1]) & (a[..., 0] >= a[..., 2]), 0, np.where(a[..., 1] >= a[..., 2], 1, 2))
    assert np.array_equal(major, np.broadcast_to(np.array([0, 0, 1, 1, 2, 2])[:, None, None], major.shape))


def test_the_tap_tables():
    for kind, roughness, n in ((GGX, 0.25, 64), (GGX, 1.0, 64), (GGX, 0.5, 1), (GGX, 0.7, 4096), (COSINE, 0.0, 256), (COSINE, 0.3, 63)):
        got = brt.envmap_taps(kind, roughness, n)
        want = er.taps64(kind, roughness, n)
        w32 = want.astype(F32)
        ulp = np.maximum(np.abs(np.nextafter(w32, F32(np.inf)) - w32), np.abs(w32 - np.nextafter(w32, F32(-np.inf)))).astype(np.float64)
        assert got.shape == (n, 4) and (np.abs(got.astype(np.float64) - want) <= ulp).all(), (kind, roughness, n)      # (libm may differ)
        assert (got[:, 3] >= 0).all()
        length = np.sqrt((got[:, :3].astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(length - 1.0).max() < 1e-6
    assert np.array_equal(brt.envmap_taps(GGX, 0.0, 257), np.broadcast_to(np.array([0, 0, 1, 1], F32), (257, 4)))      # a mirror
    assert np.count_nonzero(_table("ggx100_64")[:, 3] > 0) in (31, 32, 33)                # roughness 1 drops half its taps
    assert (brt.envmap_taps(COSINE, 0.0, 256)[:, 3] == 1).all()
    assert np.array_equal(brt.envmap_taps(COSINE, 0.0, 64), brt.envmap_taps(COSINE, 5.0, 64))     # (the cosine table reads no roughness)
    # the chain's roughness is an f32 divide
    assert er.level_roughness(1, 4) == F32(1) / F32(3)


def test_every_host_refusal_writes_nothing():
    lib = _lib.load()
    out = np.full(6 * 16 * 16 * 4 + 8, 7.0, F32)
    src, taps = _cube("gradient", 8), _table("ggx25_64")
    o, s, t = out.ctypes.data, src.ctypes.data, taps.ctypes.data
    fp = out.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))
    calls = {
        "directions, size 0": lambda: lib.brt_host_envmap_directions(0, fp),
        "directions, size 4097": lambda: lib.brt_host_envmap_directions(4097, fp),
        "directions, null": lambda: lib.brt_host_envmap_directions(4, None),
        "taps, kind 2": lambda: lib.brt_host_envmap_taps(2, 0.5, 16, o),
        "taps, roughness -0.1": lambda: lib.brt_host_envmap_taps(GGX, -0.1, 16, o),
        "taps, roughness 1.5": lambda: lib.brt_host_envmap_taps(GGX, 1.5, 16, o),
        "taps, roughness NaN": lambda: lib.brt_host_envmap_taps(GGX, float("nan"), 16, o),
        "taps, n 0": lambda: lib.brt_host_envmap_taps(GGX, 0.5, 0, o),
        "taps, n 4097": lambda: lib.brt_host_envmap_taps(GGX, 0.5, 4097, o),
        "taps, null": lambda: lib.brt_host_envmap_taps(GGX, 0.5, 16, None),
        "downsample, odd": lambda: lib.brt_host_envmap_downsample(s, 7, o),
        "downsample, size 0": lambda: lib.brt_host_envmap_downsample(s, 0, o),
        "downsample, size 4098": lambda: lib.brt_host_envmap_downsample(s, 4098, o),
        "downsample, null src": lambda: lib.brt_host_envmap_downsample(None, 8, o),
        "downsample, null out": lambda: lib.brt_host_envmap_downsample(s, 8, None),
        "downsample, overlap": lambda: lib.brt_host_envmap_downsample(o, 8, o + 64),
        "filter, src_size 0": lambda: lib.brt_host_envmap_filter(s, 0, t, 64, 4, o),
        "filter, src_size 4097": lambda: lib.brt_host_envmap_filter(s, 4097, t, 64, 4, o),
        "filter, dst_size 0": lambda: lib.brt_host_envmap_filter(s, 8, t, 64, 0, o),
        "filter, dst_size 4097": lambda: lib.brt_host_envmap_filter(s, 8, t, 64, 4097, o),
        "filter, n_taps 0": lambda: lib.brt_host_envmap_filter(s, 8, t, 0, 4, o),
        "filter, n_taps 4097": lambda: lib.brt_host_envmap_filter(s, 8, t, 4097, 4, o),
        "filter, null src": lambda: lib.brt_host_envmap_filter(None, 8, t, 64, 4, o),
        "filter, null taps": lambda: lib.brt_host_envmap_filter(s, 8, None, 64, 4, o),
        "filter, null out": lambda: lib.brt_host_envmap_filter(s, 8, t, 64, 4, None),
        "filter, out over src": lambda: lib.brt_host_envmap_filter(o, 8, t, 64, 4, o + 256),
        "filter, out over taps": lambda: lib.brt_host_envmap_filter(s, 8, o + 32, 64, 4, o),
    }
    for what, call in calls.items():
        assert call() == INVALID, what
        assert (out == 7.0).all(), f"{what}: something was written"
        assert lib.brt_last_error(None), what
    assert np.array_equal(brt.envmap_filter_host(src, taps, 4).view(np.uint32), _want("gradient", 8, 4, "ggx25_64")[0].view(np.uint32))


@pytest.mark.parametrize("pair", PAIRS)
def test_the_host_filter_is_the_restatement(pair):
    src, dst = pair
    up_x = False
    for kind in CUBES:
        for table in TABLES:
            want, info = _want(kind, src, dst, table)
            got = brt.envmap_filter_host(_cube(kind, src), _table(table), dst)
            assert_texels_equal(got, want, f"{kind} {pair} {table}")
            if table == "zero_64":
                assert not got.any() and not np.signbit(got).any()
                continue
            # the fixture is not vacuous: every face is reached, and the clamp at a face edge is taken
            assert info["faces"] == set(range(6)) and info["up_z"], (kind, pair, table)
            assert info["clamped"] or table == "one", (kind, pair, table)
            up_x |= info["up_x"]
            if table == "nanw_64":
                assert not want.any()                     # (sw is a NaN, and a NaN is not > 0: step 12 gives 0)
            elif kind == "special" and src >= 8:
                assert np.isnan(want).any() and (np.isfinite(want).any() or dst < 16)
            elif kind == "constant":
                assert (np.abs(got.astype(np.float64) - np.array(CONSTANT)) <= ACROSS_ROUNDINGS * np.maximum(1.0, np.array(CONSTANT))).all()
    # both branches of the frame: a destination texel within 0.999 of +-z exists at the odd sizes (the face centres) and at 1
    assert up_x == (dst in (1, 3, 5)), pair


def test_both_branches_of_the_frame_are_taken_over_the_pairs():
    assert any(_want("gradient", s, d, "ggx25_64")[1]["up_x"] for s, d in PAIRS) and all(_want("gradient", s, d, "ggx25_64")[1]["up_z"] for s, d in PAIRS)


@pytest.mark.parametrize("size", [2, 8, 16, 18])
def test_the_host_downsample_is_the_restatement(size):
    for kind in CUBES:
        got = brt.envmap_downsample_host(_cube(kind, size))
        want = er.downsample(_cube(kind, size))
        assert got.shape == (6, size // 2, size // 2, 4)
        assert_texels_equal(got, want, f"{kind} {size}")
        if kind == "constant":
            assert np.array_equal(got, _cube(kind, size // 2))
        if kind == "special":
            assert np.isnan(want).any() and np.isfinite(want).any()


def test_the_host_twins_read_and_write_buffers_at_any_address():
    lib = _lib.load()
    src, taps, want = _cube("special", 8), _table("ggx25_63"), _want("special", 8, 4, "ggx25_63")[0]
    for shift in (1, 2, 3, 4, 8):
        raw_src = np.zeros(src.nbytes + 16, np.uint8)
        raw_taps = np.zeros(taps.nbytes + 16, np.uint8)
        raw_out = np.zeros(want.nbytes + 16, np.uint8)
        raw_src[shift:shift + src.nbytes] = src.view(np.uint8).reshape(-1)
        raw_taps[shift:shift + taps.nbytes] = taps.view(np.uint8).reshape(-1)
        assert lib.brt_host_envmap_filter(raw_src.ctypes.data + shift, 8, raw_taps.ctypes.data + shift, 63, 4, raw_out.ctypes.data + shift) == 0
        assert_texels_equal(raw_out[shift:shift + want.nbytes].copy().view(F32).reshape(want.shape), want, f"filter at +{shift}")
        assert not raw_out[:shift].any() and not raw_out[shift + want.nbytes:].any()
        half = er.downsample(src)
        raw_out[:] = 0
        assert lib.brt_host_envmap_downsample(raw_src.ctypes.data + shift, 8, raw_out.ctypes.data + shift) == 0
        assert_texels_equal(raw_out[shift:shift + half.nbytes].copy().view(F32).reshape(half.shape), half, f"downsample at +{shift}")
        raw_dir = np.zeros(6 * 9 * 12 + 16, np.uint8)
        assert lib.brt_host_envmap_directions(3, _lib.C.cast(raw_dir.ctypes.data + shift, _lib.C.POINTER(_lib.C.c_float))) == 0
        assert raw_dir[shift:shift + 648].tobytes() == er.directions(3).tobytes()
        raw_t = np.zeros(63 * 16 + 16, np.uint8)
        assert lib.brt_host_envmap_taps(GGX, 0.25, 63, raw_t.ctypes.data + shift) == 0
        assert raw_t[shift:shift + 63 * 16].tobytes() == taps.tobytes()


def test_the_f32_rule_against_float64():
    worst = 0.0
    for kind in ("constant", "lit", "gradient"):
        for src, dst in PAIRS:
            for table in ("one", "ggx25_63", "ggx25_64", "ggx25_65", "ggx100_64", "cosine_256"):
                f32 = _want(kind, src, dst, table)[0]
                f64 = er.filter_cube(_cube(kind, src), _table(table), dst, np.float64)
                e = _rel(f32, f64).max()
                worst = max(worst, e)
                print(f"{kind} {src}->{dst} {table}: {e:.3e}")
    print(f"largest |f32 - float64| / max(1, |ref|): {worst:.3e}")
    assert worst <= F32_VS_F64
    # the library's twin against the float64 rule, four times as much
    for src, dst in PAIRS:
        got = brt.envmap_filter_host(_cube("gradient", src), _table("cosine_256"), dst)
        assert _rel(got, er.filter_cube(_cube("gradient", src), _table("cosine_256"), dst, np.float64)).max() <= ACROSS_ROUNDINGS


@functools.lru_cache(maxsize=None)
def _sky_cube(size):
    """The analytic sky, linear: A + B d_y per channel, alpha 0 (a miss)."""
    d = er.directions(size).astype(np.float64)
    c = np.zeros((6, size, size, 4), F32)
    c[..., :3] = SKY_A + SKY_B * d[..., 1:2]
    c.setflags(write=False)
    return c


def _sky_cosine_error(filtered, size):
    n = er.directions(size).astype(np.float64)
    want = SKY_A + (2.0 / 3.0) * SKY_B * n[..., 1:2]
    return np.abs(filtered[..., :3].astype(np.float64) - want).max()


def test_the_cosine_map_of_the_analytic_sky():
    sky, cosine = _sky_cube(16), _table("cosine_256")
    measured = _sky_cosine_error(er.filter_cube(sky, cosine, 16), 16)
    print(f"f32 restatement, cosine 256 taps on the 16 x 16 sky cube: largest |filter - (A + 2/3 B n_y)| {measured:.3e}")
    assert 0.5 * SKY_COSINE_ERROR <= measured <= SKY_COSINE_ERROR                       # (the figure the bound is made from)
    got = brt.envmap_filter_host(sky, cosine, 16)
    assert _sky_cosine_error(got, 16) <= SKY_COSINE_BOUND
    assert not got[..., 3].any()                                                          # the sky's alpha stays 0
    more = _sky_cosine_error(brt.envmap_filter_host(sky, brt.envmap_taps(COSINE, 0.0, 1024), 16), 16)
    print(f"1024 taps: {more:.3e}")
    assert more < measured


def test_the_stand_alone_twin_under_sanitizers(tmp_path):
    """tests/tools/envmap_twin_main.hip: the host rule alone in a program of its own, built with the address and undefined-behaviour
    sanitizers and run on the CPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "envmap_twin_main")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "bevyray_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "tools", "envmap_twin_main.hip")]
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


def _filter_device(plugin, src, taps, dst, stream=None):
    d_src, d_taps = _dev(src), _dev(taps)
    n = 6 * dst * dst * 16
    d_out = _guarded(n, 32, 0xCD)
    plugin.node.envmap_filter_device(d_src.data_ptr(), src.shape[1], d_taps.data_ptr(), len(taps), dst, d_out.data_ptr(), stream=stream)
    return _read(d_out, n, 0xCD, "filter").view(F32).reshape(6, dst, dst, 4)


def _downsample_device(plugin, src):
    s = src.shape[1]
    n = 6 * (s // 2) ** 2 * 16
    d_src, d_out = _dev(src), _guarded(n, 32, 0xCD)
    plugin.node.envmap_downsample_device(d_src.data_ptr(), s, d_out.data_ptr())
    return _read(d_out, n, 0xCD, "downsample").view(F32).reshape(6, s // 2, s // 2, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 3, 8, 11])
def test_generated_rays_are_the_host_directions_and_seeds(plugin, size):
    n = 6 * size * size
    for position, seed in (((0.5, -1.25, 3.0), 0xFFFFFF00), ((-0.0, 1e-42, -3e38), 5)):
        d_rays = _guarded(n * 32, 32, 0xAB)
        plugin.node.envmap_rays_device(position, seed, size, d_rays.data_ptr())
        got = _read(d_rays, n * 32, 0xAB, "rays").view(brt.RADIANCE_RAY_DTYPE)
        assert np.array_equal(got["origin"].view(np.uint32), np.broadcast_to(np.array(position, F32), (n, 3)).view(np.uint32))
        assert np.array_equal(got["direction"].view(np.uint32), brt.envmap_directions(size).reshape(n, 3).view(np.uint32))
        assert np.array_equal(got["direction"].view(np.uint32), er.directions(size).reshape(n, 3).view(np.uint32))
        assert np.array_equal(got["seed"], er.seeds(seed, size)) and np.array_equal(got["user"], np.arange(n, dtype=np.uint32))


@pytest.mark.gpu
def test_the_resolve_kernel_on_synthetic_results(plugin):
    for size in (1, 3, 8):
        n = 6 * size * size
        rng = np.random.default_rng([62, size])
        res = np.zeros(n, brt.RADIANCE_DTYPE)
        res["t"] = rng.uniform(0, 50, n)
        res["rgb"] = rng.uniform(0, 2, size=(n, 3)).astype(F32)
        res["status"] = rng.choice([0, 1, 3, 4, 8], size=n)
        res["sphere"], res["material"], res["user"] = 0xFFFFFFFF, 7, np.arange(n)
        for k, v in enumerate((np.nan, np.inf, -np.inf, 3e38, 1e-30, -0.0)):
            res["rgb"][k % n, k % 3] = v
        d_res, d_out = _dev(res), _guarded(n * 16, 32, 0xCD)
        plugin.node.envmap_resolve_device(d_res.data_ptr(), size, d_out.data_ptr())
        got = _read(d_out, n * 16, 0xCD, "resolve").view(F32).reshape(n, 4)
        assert_texels_equal(got, er.resolve(res["rgb"], res["status"]), f"size {size}")
        assert np.array_equal(got[:, 3] == 1.0, (res["status"] & 1) != 0) and set(np.unique(got[:, 3])) <= {0.0, 1.0}


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_the_filter_kernel_is_the_host_twin_and_the_restatement(plugin, pair):
    src, dst = pair
    for kind in CUBES:
        for table in TABLES:
            got = _filter_device(plugin, _cube(kind, src), _table(table), dst)
            what = f"{kind} {pair} {table}"
            assert_texels_equal(got, _want(kind, src, dst, table)[0], what)
            assert_texels_equal(got, brt.envmap_filter_host(_cube(kind, src), _table(table), dst), what + ", twin")


@pytest.mark.gpu
@pytest.mark.parametrize("size", [2, 8, 16, 18])
def test_the_downsample_kernel_is_the_host_twin_and_the_restatement(plugin, size):
    for kind in CUBES:
        got = _downsample_device(plugin, _cube(kind, size))
        assert_texels_equal(got, er.downsample(_cube(kind, size)), f"{kind} {size}")
        assert_texels_equal(got, brt.envmap_downsample_host(_cube(kind, size)), f"{kind} {size}, twin")


POSITION, SEED, SIZE, LEVELS, TAPS, BOUNCES = (2.5, 1.5, 3.5), 0xFFFFFFC0, 8, 4, 64, 8
PLAIN, STREAM = 1, 2


def _steps(plugin, position, seed, size, levels, samples, bounces, n_taps, **knobs):
    """The chain through the step exports: rays -> brt_radiance_rays_device -> resolve, then per level downsample -> filter with the
    exported table.  -> (the (n, 4) chain, the radiance results, the radiance call's stats)."""
    import torch
    n = 6 * size * size
    offs = er.level_offsets(size, levels)
    d_rays, d_res = _guarded(n * 32, 32, 0xAB), _guarded(n * 32, 32, 0xAB)
    d_chain = _guarded(offs[-1] * 16, 32, 0xCD)
    plugin.node.envmap_rays_device(position, seed, size, d_rays.data_ptr())
    with plugin.tuning(**knobs):
        rad = dict(plugin.node.radiance_rays((d_rays.data_ptr(), n, d_res.data_ptr()), samples, bounces, device=True))
    plugin.node.envmap_resolve_device(d_res.data_ptr(), size, d_chain.data_ptr())
    box_ptr = d_chain.data_ptr()
    keep = []
    for l in range(1, levels):
        s = size >> l
        d_next = _guarded(6 * s * s * 16, 32, 0xEE)
        d_taps = _dev(brt.envmap_taps(GGX, er.level_roughness(l, levels), n_taps))
        plugin.node.envmap_downsample_device(box_ptr, 2 * s, d_next.data_ptr())
        plugin.node.envmap_filter_device(d_next.data_ptr(), s, d_taps.data_ptr(), n_taps, s, d_chain.data_ptr() + offs[l] * 16)
        keep += [d_next, d_taps]
        box_ptr = d_next.data_ptr()
    chain = _read(d_chain, offs[-1] * 16, 0xCD, "chain").view(F32).reshape(-1, 4)
    results = _read(d_res, n * 32, 0xAB, "results").view(brt.RADIANCE_DTYPE)
    return chain, results, rad


def _bake_device(plugin, position, seed, size, levels, samples, bounces, n_taps, out_format=0, stream=None, **knobs):
    offs = er.level_offsets(size, levels)
    texel = 8 if out_format == brt.FLAG_OUT_RGBA16F else 16
    d_out = _guarded(offs[-1] * texel, 32, 0xCD)
    with plugin.tuning(**knobs):
        st = dict(plugin.node.bake_envmap(position, size, levels, samples, bounces, n_taps, seed, d_out=d_out.data_ptr(), stream=stream,
                                          out_format=out_format))
    got = _read(d_out, offs[-1] * texel, 0xCD, "bake").view(np.float16 if texel == 8 else F32).reshape(-1, 4)
    return got, st


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("tree", ["caller", "callee"])
def test_a_bake_is_the_radiance_call_the_restated_resolve_and_its_own_steps(plugin, tree, samples):
    _upload_cover(plugin, tree)
    n = 6 * SIZE * SIZE
    three_chunks = {"BRT_PROBE_CHUNK_RAYS": n // 3}
    want, results, rad = _steps(plugin, POSITION, SEED, SIZE, LEVELS, samples, BOUNCES, TAPS)
    # level 0: the radiance call over the host-built list, resolved by the restatement
    rays = rr.make_rays(np.broadcast_to(np.array(POSITION, F32), (n, 3)), er.directions(SIZE).reshape(n, 3), er.seeds(SEED, SIZE),
                        np.arange(n, dtype=np.uint32))
    host_results = plugin.node.radiance_rays(rays, samples, BOUNCES)
    rr.assert_equal(results, host_results, "the generated list")
    level0 = er.resolve(host_results["rgb"], host_results["status"])
    hit = (host_results["status"] & 1) != 0
    assert 20 < hit.sum() < n - 20 and len(np.unique(level0[:, 0])) > n // 4                 # (the cube sees spheres and sky)
    assert_texels_equal(want[:n], level0, "level 0")
    # ... and the chain is the restatement's over that level 0 and the exported tables
    tables = [brt.envmap_taps(GGX, er.level_roughness(l, LEVELS), TAPS) for l in range(1, LEVELS)]
    assert_texels_equal(want, er.chain(level0.reshape(6, SIZE, SIZE, 4), LEVELS, tables), "the chain")
    assert (want[er.level_offsets(SIZE, LEVELS)[1]:] != 0).any()
    seen = {}
    for form in (PLAIN, STREAM):
        for chunks, knobs in ((1, {}), (3, three_chunks)):
            got, st = _bake_device(plugin, POSITION, SEED, SIZE, LEVELS, samples, BOUNCES, TAPS, BRT_RADIANCE_FORM=form, **knobs)
            what = f"{tree} samples {samples} form {form} chunks {chunks}"
            assert_texels_equal(got, want, what)
            assert (st["walks"], st["hits"], st["refused"], st["chunks"], st["form"]) == (rad["walks"], int(hit.sum()), 0, chunks, form - 1), (what, st, rad)
            with plugin.tuning(BRT_RADIANCE_FORM=form, **knobs):
                host = plugin.node.bake_envmap(POSITION, SIZE, LEVELS, samples, BOUNCES, TAPS, SEED)
            assert_texels_equal(host, want, what + ", host")
            assert plugin.node.last_probe_stats == st, what
            half, st16 = _bake_device(plugin, POSITION, SEED, SIZE, LEVELS, samples, BOUNCES, TAPS, brt.FLAG_OUT_RGBA16F, BRT_RADIANCE_FORM=form, **knobs)
            assert_texels_equal(half, want.astype(np.float16), what + ", RGBA16F")
            assert st16 == st
            seen[form, chunks] = got.tobytes()
    with plugin.tuning(**three_chunks):
        host16 = plugin.node.bake_envmap(POSITION, SIZE, LEVELS, samples, BOUNCES, TAPS, SEED, out_format=brt.FLAG_OUT_RGBA16F)
    assert_texels_equal(host16, want.astype(np.float16), "host, RGBA16F")
    assert len(set(seen.values())) == 1
    # fewer levels are a prefix of level 0 only: the roughness of a level depends on `levels`
    one, _ = _bake_device(plugin, POSITION, SEED, SIZE, 1, samples, BOUNCES, TAPS)
    assert_texels_equal(one, want[:n], "levels = 1")


@pytest.mark.gpu
def test_an_empty_sky(plugin):
    plugin.node.write_buffers(make_buffers([((300.0, 400.0, 500.0), 0.01, brt.StandardMaterial())]))
    size = 16
    n = 6 * size * size
    got, st = _bake_device(plugin, (0.5, 1.0, -2.0), 9, size, 3, 1, 8, 64)
    assert (st["hits"], st["refused"], st["walks"]) == (0, 0, n)
    d = er.directions(size).reshape(n, 3)
    sky = rr.sky_rgb(d)                                                 # bitwise, as tests/test_radiance.py holds a miss ray to it
    want0 = np.concatenate([(sky * sky).astype(F32), np.zeros((n, 1), F32)], axis=1)
    assert np.array_equal(got[:n].view(np.uint32), want0.view(np.uint32))
    assert np.abs(got[:n, :3].astype(np.float64) - (SKY_A + SKY_B * d[:, 1:2].astype(np.float64))).max() < 1e-6
    assert not got[:, 3].any()
    # the diffuse map: the cosine table over level 0, against the closed form within the bound of the CPU test
    level0 = got[:n].reshape(6, size, size, 4)
    cosine = _table("cosine_256")
    diffuse = _filter_device(plugin, level0, cosine, size)
    assert_texels_equal(diffuse, er.filter_cube(level0, cosine, size), "the diffuse map")
    err = _sky_cosine_error(diffuse, size)
    print(f"cosine map of the traced sky: largest |filter - (A + 2/3 B n_y)| {err:.3e}")
    assert err <= SKY_COSINE_BOUND


@pytest.mark.gpu
def test_a_scene_with_32_bit_descriptors(plugin):
    s = big_scene(16383, 11)
    b = brt.Buffers(s.models, s.materials, brt.build_bvh(s.models))
    lvl, cam, win = big_view(96, 54)
    plugin.node.run(lvl, cam, win, 96, 54, buffers=b)
    assert plugin.node.last_stats["scene_in_lds"] == 0
    centre = tuple(float(x) for x in b.models["position"].astype(np.float64).mean(axis=0))
    want, results, rad = _steps(plugin, centre, 77, SIZE, LEVELS, 1, 4, TAPS)
    assert rad["hits"] > 50 and rad["form"] == 0
    got, st = _bake_device(plugin, centre, 77, SIZE, LEVELS, 1, 4, TAPS, BRT_PROBE_CHUNK_RAYS=100)
    assert_texels_equal(got, want, "32-bit descriptors")
    assert st["form"] == 0 and st["chunks"] == 4 and (st["walks"], st["hits"]) == (rad["walks"], rad["hits"])     # (no LDS form: the plain kernel)
    with plugin.tuning(BRT_RADIANCE_FORM=STREAM):
        assert_texels_equal(plugin.node.bake_envmap(centre, SIZE, LEVELS, 1, 4, TAPS, 77), want, "streaming")
        assert plugin.node.last_probe_stats["form"] == 1


@pytest.mark.gpu
def test_host_bakes_behind_a_held_bake_rewrite_the_table_and_share_the_io_buffer(plugin):
    """The tap table and the host forms' io buffer change under a bake in flight.  A device bake of an 8 x 8 cube with 3 levels and 16
    taps in chunks of 128 texels (384 texels: three chunks) is held on a caller's stream of a new context; with no host synchronisation
    the host bake of another (levels, n_taps) pair then rewrites the tap table behind it and allocates the io buffer, the host bake of
    27 probes x 64 directions uploads the direction table for the first time and takes the io buffer over, and the host bake of a
    2 x 2 x 2 lattice takes it over again.  The smallest shapes at which the bake chunks, the table's key changes and the io buffer
    changes owner.  Expectations: the same four calls one at a time on the module's context."""
    import torch
    _upload_cover(plugin, "caller")
    held = (POSITION, SEED, 8, 3, 1, 4, 16)
    g = [np.linspace(lo, hi, 3) for lo, hi in ((-5.0, 5.0), (0.1, 3.0), (-5.0, 5.0))]
    probes = np.zeros(27, brt.PROBE_DTYPE)
    probes["position"] = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    probes["seed"] = np.arange(27, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(1)
    vol = brt.make_volume((-3.0, 0.5, -3.0), (6.0, 2.0, 6.0), (2, 2, 2), brt.PROBE_SH9, 0xFFFFFFF0, 0)

    def host_calls(p):
        return (p.node.bake_envmap(POSITION, 8, 4, 1, 4, 8, SEED).copy(), p.node.bake_probes(probes, 64, 4, brt.PROBE_SH9).copy(),
                p.node.bake_volume(vol, 64, 4).copy())

    want_held, st = _bake_device(plugin, *held, BRT_PROBE_CHUNK_RAYS=128)
    assert st["chunks"] == 3
    want_env, want_probes, want_vol = host_calls(plugin)
    assert want_held[:, 3].any() and want_env[:, 3].any() and want_probes["hits"].any() and want_vol["hits"].any() and len(want_vol) == 8
    n = er.level_offsets(8, 3)[-1] * 16
    d_out = _guarded(n, 32, 0xCD)
    sa = torch.cuda.Stream()
    fresh = brt.RaytracePlugin([0])
    try:
        fresh.node.write_buffers(_cover())
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(20_000_000)                       # (a few ms: the held bake starts after the later calls have been made)
        with fresh.tuning(BRT_PROBE_CHUNK_RAYS=128):
            st = fresh.node.bake_envmap(POSITION, 8, 3, 1, 4, 16, SEED, d_out=d_out.data_ptr(), stream=sa.cuda_stream)
        assert st["chunks"] == 3
        got_env, got_probes, got_vol = host_calls(fresh)
        assert_texels_equal(got_env, want_env, "the host bake of another pair")
        assert got_probes.tobytes() == want_probes.tobytes() and got_vol.tobytes() == want_vol.tobytes()
        assert_texels_equal(_read(d_out, n, 0xCD, "the held bake").view(F32).reshape(-1, 4), want_held, "the held bake")
    finally:
        fresh.close()


@pytest.mark.gpu
def test_streams_uploads_frames_and_refusals(plugin):
    import torch
    b = _cover()
    w, h = 160, 90
    lvl, cam, win = brt.cover_camera(w, h, 2, 4, brt.Raytracing.Pure, 0.5)
    before = plugin.node.run(lvl, cam, win, w, h, buffers=b, flags=brt.FLAG_COUNTERS).copy()
    stats_before = dict(plugin.node.last_stats)
    args = (POSITION, SEED, SIZE, LEVELS, 1, 4, TAPS)
    serial, _ = _bake_device(plugin, *args)
    offs = er.level_offsets(SIZE, LEVELS)
    n = offs[-1]
    cosine = _table("cosine_256")
    diffuse = er.filter_cube(serial[:offs[1]].reshape(6, SIZE, SIZE, 4), cosine, 4)
    # a bake on one caller stream, the diffuse filter of its level 0 on another: the same bytes
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_chain = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_taps, d_diff = _dev(cosine), torch.zeros(6 * 16 * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def on_two_streams(between=None):
        d_chain.zero_()
        d_diff.zero_()
        torch.cuda.synchronize()
        st = plugin.node.bake_envmap(POSITION, SIZE, LEVELS, 1, 4, TAPS, SEED, d_out=d_chain.data_ptr(), stream=s1.cuda_stream)
        assert (st["walks"], st["hits"], st["refused"], st["chunks"]) == (0, 0, 0, 1)
        if between:
            between()
        plugin.node.envmap_filter_device(d_chain.data_ptr(), SIZE, d_taps.data_ptr(), len(cosine), 4, d_diff.data_ptr(), stream=s2.cuda_stream)
        torch.cuda.synchronize()
        assert_texels_equal(d_chain.cpu().numpy().view(F32).reshape(-1, 4), serial, "two streams")
        assert_texels_equal(d_diff.cpu().numpy().view(F32).reshape(6, 4, 4, 4), diffuse, "two streams, the diffuse map")

    on_two_streams()
    # an upload between the bake and the filter waits for the bake and changes nothing in either
    moved = b.models.copy()
    moved["position"][np.flatnonzero(moved["radius"] == 1.0)] += np.array([0.0, 0.6, 0.0], F32)
    on_two_streams(lambda: plugin.node.write_buffers(brt.Buffers(moved, b.materials, brt.build_bvh(moved))))
    assert _bake_device(plugin, *args)[0].tobytes() != serial.tobytes()                       # (the new scene bakes another cube)
    plugin.node.write_buffers(b)

    # every refusal writes nothing and is followed by a correct call
    lib, ctx = plugin._lib, plugin._ctx
    d_buf = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")
    A = d_buf.data_ptr()
    B = A + (1 << 19)
    pos = (_lib.C.c_float * 3)(*POSITION)
    nan_pos = (_lib.C.c_float * 3)(0.0, float("nan"), 0.0)
    inf_pos = (_lib.C.c_float * 3)(float("inf"), 0.0, 0.0)
    host_out = np.full((n, 4), 3.0, F32)
    H = host_out.ctypes.data

    def refused(code, call, what):
        assert call() == code, what
        torch.cuda.synchronize()
        assert bool((d_buf == 0x5A).all()) and (host_out == 3.0).all(), f"{what}: something was written"
        assert_texels_equal(_bake_device(plugin, *args)[0], serial, f"after {what}")

    def bake(position=pos, size=SIZE, levels=LEVELS, samples=1, bounces=4, taps=TAPS, bound=0.0, out=A, flags=0):
        return lambda: lib.brt_bake_envmap_device(ctx, position, SEED, size, levels, samples, bounces, taps, bound, out, None, flags, None)

    refused(INVALID, bake(position=nan_pos), "a NaN position")
    refused(INVALID, bake(position=inf_pos), "an INF position")
    refused(INVALID, bake(position=None), "no position")
    refused(INVALID, bake(size=0), "size 0")
    refused(INVALID, bake(size=12), "a size that is no power of two")
    refused(INVALID, bake(size=2048), "size 2048")
    refused(INVALID, bake(levels=0), "levels 0")
    refused(INVALID, bake(levels=5), "levels 5 of size 8")
    refused(INVALID, bake(samples=0), "samples 0")
    refused(INVALID, bake(samples=65536), "samples 65536")
    refused(INVALID, bake(bounces=65536), "bounces 65536")
    refused(INVALID, bake(taps=0), "n_taps 0")
    refused(INVALID, bake(taps=4097), "n_taps 4097")
    refused(INVALID, bake(bound=float("nan")), "origin_bound NaN")
    refused(INVALID, bake(bound=-1.0), "origin_bound < 0")
    refused(INVALID, bake(out=None), "null out")
    refused(INVALID, bake(out=A + 8), "out not 16-byte aligned")
    refused(INVALID, bake(flags=brt.FLAG_DENOISE), "an unknown flag")
    refused(INVALID, bake(flags=brt.FLAG_OUT_RGBA8_UNORM), "another output format")
    refused(INVALID, lambda: lib.brt_bake_envmap(ctx, pos, SEED, SIZE, LEVELS, 1, 4, TAPS, 0.0, None, 0, None), "host, null out")
    refused(INVALID, lambda: lib.brt_bake_envmap(ctx, nan_pos, SEED, SIZE, LEVELS, 1, 4, TAPS, 0.0, H, 0, None), "host, a NaN position")
    refused(INVALID, lambda: lib.brt_bake_envmap(ctx, pos, SEED, SIZE, LEVELS, 1, 4, TAPS, 0.0, H, brt.FLAG_CALLER_STREAM, None), "host, a flag")
    refused(INVALID, lambda: lib.brt_envmap_rays_device(ctx, nan_pos, 1, 4, A, None, 0), "rays, a NaN position")
    refused(INVALID, lambda: lib.brt_envmap_rays_device(ctx, pos, 1, 0, A, None, 0), "rays, size 0")
    refused(INVALID, lambda: lib.brt_envmap_rays_device(ctx, pos, 1, 4097, A, None, 0), "rays, size 4097")
    refused(INVALID, lambda: lib.brt_envmap_rays_device(ctx, pos, 1, 4, None, None, 0), "rays, null")
    refused(INVALID, lambda: lib.brt_envmap_rays_device(ctx, pos, 1, 4, A + 4, None, 0), "rays, not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_envmap_rays_device(ctx, pos, 1, 4, A, None, brt.FLAG_COUNTERS), "rays, an unknown flag")
    refused(INVALID, lambda: lib.brt_envmap_resolve_device(ctx, A, 0, B, None, 0), "resolve, size 0")
    refused(INVALID, lambda: lib.brt_envmap_resolve_device(ctx, None, 4, B, None, 0), "resolve, null results")
    refused(INVALID, lambda: lib.brt_envmap_resolve_device(ctx, A, 4, None, None, 0), "resolve, null out")
    refused(INVALID, lambda: lib.brt_envmap_resolve_device(ctx, A, 4, A + 64, None, 0), "resolve, overlap")
    refused(INVALID, lambda: lib.brt_envmap_resolve_device(ctx, A + 8, 4, B, None, 0), "resolve, not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_envmap_resolve_device(ctx, A, 4, B, None, brt.FLAG_OUT_RGBA16F), "resolve, an unknown flag")
    refused(INVALID, lambda: lib.brt_envmap_downsample_device(ctx, A, 7, B, None, 0), "downsample, odd")
    refused(INVALID, lambda: lib.brt_envmap_downsample_device(ctx, A, 0, B, None, 0), "downsample, size 0")
    refused(INVALID, lambda: lib.brt_envmap_downsample_device(ctx, None, 8, B, None, 0), "downsample, null")
    refused(INVALID, lambda: lib.brt_envmap_downsample_device(ctx, A, 8, A + 1024, None, 0), "downsample, overlap")
    refused(INVALID, lambda: lib.brt_envmap_downsample_device(ctx, A, 8, B + 4, None, 0), "downsample, not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_envmap_downsample_device(ctx, A, 8, B, None, brt.FLAG_DENOISE), "downsample, an unknown flag")
    T = A + (1 << 18)
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 0, T, 64, 4, B, None, 0), "filter, src_size 0")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, T, 64, 4097, B, None, 0), "filter, dst_size 4097")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, T, 0, 4, B, None, 0), "filter, n_taps 0")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, T, 4097, 4, B, None, 0), "filter, n_taps 4097")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, None, 8, T, 64, 4, B, None, 0), "filter, null src")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, None, 64, 4, B, None, 0), "filter, null taps")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, T, 64, 4, None, None, 0), "filter, null out")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, T, 64, 4, A + 256, None, 0), "filter, out over src")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, T, 64, 4, T + 16, None, 0), "filter, out over taps")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, T + 8, 64, 4, B, None, 0), "filter, not 16-byte aligned")
    refused(INVALID, lambda: lib.brt_envmap_filter_device(ctx, A, 8, T, 64, 4, B, None, brt.FLAG_TEMPORAL), "filter, an unknown flag")
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        assert bake()() == UNSUPPORTED
        assert lib.brt_bake_envmap(ctx, pos, SEED, SIZE, LEVELS, 1, 4, TAPS, 0.0, H, 0, None) == UNSUPPORTED
    finally:
        plugin.set_policy(0)
    torch.cuda.synchronize()
    assert bool((d_buf == 0x5A).all()) and (host_out == 3.0).all(), "a bake under a policy wrote something"
    assert_texels_equal(_bake_device(plugin, *args)[0], serial, "after the bakes under a policy")
    # a position beyond the tree's bound after the reach step (a callee-built tree has a finite one)
    _upload_cover(plugin, "callee")
    bound = plugin.node.query_origin_bound()
    far = (_lib.C.c_float * 3)(2.0 * bound, 0.0, 0.0)
    callee, _ = _bake_device(plugin, *args)
    assert lib.brt_bake_envmap_device(ctx, far, SEED, SIZE, LEVELS, 1, 4, TAPS, 0.0, A, None, 0, None) == INVALID
    assert lib.brt_bake_envmap(ctx, far, SEED, SIZE, LEVELS, 1, 4, TAPS, 0.0, H, 0, None) == INVALID
    torch.cuda.synchronize()
    assert bool((d_buf == 0x5A).all()) and (host_out == 3.0).all()
    assert_texels_equal(_bake_device(plugin, *args)[0], callee, "after a position out of reach")
    plugin.node.write_buffers(b)
    with brt.RaytracePlugin([0]) as empty:
        for call in (lambda: empty.node.bake_envmap(POSITION, SIZE, LEVELS, 1, 4, TAPS, SEED),
                     lambda: empty.node.bake_envmap(POSITION, SIZE, LEVELS, 1, 4, TAPS, SEED, d_out=B)):
            with pytest.raises(brt.BrtError) as e:
                call()
            assert e.value.code == NO_SCENE
        d_t, d_s, d_o = _dev(cosine), _dev(serial[:offs[1]]), torch.zeros(6 * 16 * 16, dtype=torch.uint8, device="cuda")
        empty.node.envmap_filter_device(d_s.data_ptr(), SIZE, d_t.data_ptr(), len(cosine), 4, d_o.data_ptr())     # the steps need no scene
        assert_texels_equal(d_o.cpu().numpy().view(F32).reshape(6, 4, 4, 4), diffuse, "without a scene")
        empty.node.write_buffers(b)
        assert_texels_equal(empty.node.bake_envmap(POSITION, SIZE, LEVELS, 1, 4, TAPS, SEED), serial, "another context")
    assert bool((d_buf == 0x5A).all())

    # a plain frame after all of it is the frame before
    after = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_COUNTERS)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    for k in ("rays", "node_pops", "interior_visits", "sphere_tests", "hits", "kernel_variant", "n_workgroups", "scene_in_lds"):
        assert plugin.node.last_stats[k] == stats_before[k], k
