"""Upsampling of blended (level 1 / 2) frames (brt_upscale_blend_device, brt_render_upscaled_blend_device, brt_host_blend_covered;
DESIGN.md "Upsampling blended frames").  CPU: the exports, the argument checks, the host rule against its numpy statement
(tests/upscale_blend_ref.py), the class shares of the raster fixture from the oracle's raycast, properties of the restatement.  GPU: the
covered set, the covered texels and the uncovered pixels exactly, in the four store formats; the frame against the restatement; the
one-call form against its steps; level 3; edge inputs; unchanged paths; streams; refusals.

The fixture (upscale_blend_ref.raster_depth / raster_rgba) on the cover scene with the camera of tests/test_upscale.py's _view: covered
share 0.41 - 0.44 at both levels at every size used here (the CPU test prints and holds them), so both classes hold at least 20 %."""
import ctypes

import numpy as np
import pytest

import bevyray_amd as brt
from bevyray_amd import _lib
import denoise_ref as dr
import upscale_blend_ref as ubr
import upscale_ref as ur
from helpers import uniforms

F32 = np.float32
ERR_INVALID, ERR_NO_SCENE, ERR_UNSUPPORTED = -1, -7, -8
SHAPES = [(96, 54, 48, 27), (41, 23, 21, 12), (161, 91, 41, 23), (1, 1, 1, 1)]
SHAPE_IDS = ["%dx%d_from_%dx%d" % s for s in SHAPES]
LEVELS = {1: brt.Raytracing.FallbackRaster, 2: brt.Raytracing.FallbackRaytraced, 3: brt.Raytracing.Pure}
FORMATS = ((brt.FLAG_OUT_RGBA32F, None), (brt.FLAG_OUT_RGBA8_UNORM_SRGB, "srgb8"), (brt.FLAG_OUT_RGBA8_UNORM, "unorm8"),
           (brt.FLAG_OUT_RGBA16F, "f16"))
MIN_SHARE = 0.20


def _view(w, h, spp=2, level=3, seed=0.5):
    """The camera of tests/test_upscale.py's _view, with the level of the presented frame."""
    return uniforms(w, h, spp, 2, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0), 0.5, seed, level=LEVELS[level])


def _assert_shares(cov):
    c, u = ubr.class_shares(cov)
    assert c >= MIN_SHARE and u >= MIN_SHARE, (c, u)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_blend_exports_exist():
    lib = _lib.load()
    for name in ("brt_upscale_blend_device", "brt_render_upscaled_blend_device", "brt_host_blend_covered"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.brt_abi_version() == 6
    assert callable(brt.RayTracingNode.upscale_blend_device) and callable(brt.RayTracingNode.render_upscaled_blend_device)
    assert callable(brt.blend_covered)


def test_blend_argument_checks_without_a_context():
    lib = _lib.load()
    cam, win = np.zeros(80, np.uint8), np.zeros(16, np.uint8)
    c, wn = cam.ctypes.data, win.ctypes.data
    assert lib.brt_upscale_blend_device(None, c, wn, 2, 4, 4, 16, 8, 8, None, None, 4096, None, 0, None) == ERR_INVALID
    assert lib.brt_render_upscaled_blend_device(None, c, wn, 2, 4, 4, 8, 8, None, None, 4096, None, 0, None) == ERR_INVALID
    _, cam, _ = _view(8, 8)
    out = ctypes.c_uint32(7)
    assert lib.brt_host_blend_covered(None, 2, 1.0, 0.5, ctypes.byref(out)) == ERR_INVALID
    assert lib.brt_host_blend_covered(cam.ctypes.data, 2, 1.0, 0.5, None) == ERR_INVALID
    assert lib.brt_host_blend_covered(cam.ctypes.data, 0, 1.0, 0.5, ctypes.byref(out)) == ERR_UNSUPPORTED
    for level in (4, 7, 0xFFFFFFFF):
        assert lib.brt_host_blend_covered(cam.ctypes.data, level, 1.0, 0.5, ctypes.byref(out)) == ERR_INVALID
    assert out.value == 7                                              # (a refused call writes nothing)
    assert lib.brt_host_blend_covered(cam.ctypes.data, 3, 1.0, 1.0, ctypes.byref(out)) == 0 and out.value == 0


def test_host_rule_is_the_numpy_rule():
    """brt_host_blend_covered on a grid of (t, depth) pairs: t on both sides of near and far and next to them, +INF at both levels;
    depth 0, -0, negative, the values next to near / t, 1, above 1, NaN and both infinities."""
    near, far = F32(0.1), F32(1000.0)
    _, cam, _ = _view(8, 8)
    assert F32(cam[0]["near"]) == near and F32(cam[0]["far"]) == far
    ts = [0.05, 0.1, 0.65, 3.0, 7.3, 999.0, np.nextafter(far, F32(0)), far, np.nextafter(far, F32(np.inf)), 1009.0, 1010.0, 1011.0, 1e30, np.inf]
    ts = np.array(ts, F32)
    depths = [0.0, -0.0, -1.0, -1.5, 1e-6, 1e-4, 0.1 / 999.0, 0.1 / 0.65, 0.5, 1.0, 2.0, np.nan, np.inf, -np.inf]
    with np.errstate(all="ignore"):
        for t in ts:                                                   # both neighbours of every threshold near / t
            rd = near / t
            depths += [rd, np.nextafter(rd, F32(np.inf)), np.nextafter(rd, F32(-np.inf))]
    depths = np.array(depths, F32)
    tt, dd = np.meshgrid(ts, depths, indexing="ij")
    seen = set()
    for level in (1, 2):
        got = brt.blend_covered(cam, level, tt, dd)
        want = ubr.covered(cam, level, tt, dd)
        assert np.array_equal(got, want), level
        assert not got[:, np.isnan(depths)].any()                      # a NaN depth never covers
        seen.add((bool(got.any()), bool((~got).any())))
        # a miss: depth far + 10 (> far: rd = -1) at level 1, far - 1 at level 2
        miss = got[ts == np.inf][0]
        assert np.array_equal(miss, depths > (F32(-1.0) if level == 1 else near / F32(far - F32(1.0))))
    assert seen == {(True, True)}
    assert not brt.blend_covered(cam, 3, tt, dd).any()                 # level 3 never blends
    # the rule reads the camera: another near plane moves the seam
    _, cam2, _ = uniforms(8, 8, 1, 2, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0), 0.5, 0.5, near=0.4, far=50.0)
    assert np.array_equal(brt.blend_covered(cam2, 2, tt, dd), ubr.covered(cam2, 2, tt, dd))
    assert not np.array_equal(ubr.covered(cam2, 2, tt, dd), ubr.covered(cam, 2, tt, dd))


def _cover():
    return brt.generate_scene(brt.SCENE_COVER, 1)


def test_fixture_class_shares(oracle):
    """The condition every comparison of the two classes rests on: with guides from oracle_raycast alone, covered and uncovered pixels
    each hold at least 20 % of the frame at both levels and every size (1x1 aside); the NaN and the Inf texel are covered; hits in
    front of the disc's plane and behind it both occur."""
    b = _cover()
    for (w, h, _, _) in SHAPES[:3]:
        _, cam, _ = _view(w, h)
        t = dr.guides(oracle, b, cam, w, h)[..., 3]
        depth, rgba = ubr.raster_depth(w, h), ubr.raster_rgba(w, h)
        disc = (depth > 0) & (depth < 1)
        for level in (1, 2):
            cov = ubr.covered(cam, level, t, depth)
            print(f"fixture {w}x{h} level {level}: covered {ubr.class_shares(cov)[0]:.4f}, uncovered {ubr.class_shares(cov)[1]:.4f}")
            _assert_shares(cov)
            hit_disc = disc & (t < np.inf)
            assert (cov & hit_disc).any() and (~cov & hit_disc).any()
            (ny, nx), (iy, ix) = ubr.special_texels(w, h)
            assert cov[ny, nx] and cov[iy, ix] and np.isnan(rgba[ny, nx, 0]) and np.isinf(rgba[iy, ix, 1])
        # the levels differ exactly on the sky outside wall and disc
        c1, c2 = ubr.covered(cam, 1, t, depth), ubr.covered(cam, 2, t, depth)
        assert np.array_equal(c1 & ~c2, (t == np.inf) & (depth == 0)) and not (c2 & ~c1).any()


def test_restatement_covered_texels_and_uncovered_pixels(oracle):
    b = _cover()
    w, h, lw, lh = SHAPES[0]
    _, cam, _ = _view(w, h)
    g_low, g_full = dr.guides(oracle, b, cam, lw, lh), dr.guides(oracle, b, cam, w, h)
    low = np.ones((lh, lw, 4), F32)
    low[..., :3] = np.random.default_rng(11).uniform(0.25, 1.0, (lh, lw, 3)).astype(F32)
    pure, stage_pure = ur.upscale_frame(oracle, low, g_low, g_full, cam)
    depth, rgba = ubr.raster_depth(w, h), ubr.raster_rgba(w, h)
    other = np.random.default_rng(12).uniform(-2.0, 2.0, (h, w, 4)).astype(F32)
    for level in (1, 2):
        cov = ubr.covered(cam, level, g_full[..., 3], depth)
        _assert_shares(cov)
        out, stage = ubr.upscale_frame(oracle, low, g_low, g_full, cam, level, rgba, depth)
        assert np.array_equal(out[cov].view(np.uint32), rgba[cov].view(np.uint32))              # NaN and Inf included
        assert np.isnan(out[cov]).any() and np.isinf(out[cov]).any()
        assert np.array_equal(out[~cov].view(np.uint32), pure[~cov].view(np.uint32))
        assert (stage[cov] == ubr.COVERED).all() and np.array_equal(stage[~cov], stage_pure[~cov])
        out2, _ = ubr.upscale_frame(oracle, low, g_low, g_full, cam, level, other, depth)
        assert np.array_equal(out2[~cov].view(np.uint32), out[~cov].view(np.uint32))             # whatever the raster colour holds
        assert np.array_equal(out2[cov].view(np.uint32), other[cov].view(np.uint32))
        zero, _ = ubr.upscale_frame(oracle, low, g_low, g_full, cam, level, None, depth)
        assert (zero[cov] == 0).all() and not np.signbit(zero[cov]).any()
    out3, _ = ubr.upscale_frame(oracle, low, g_low, g_full, cam, 3, rgba, depth)
    assert np.array_equal(out3.view(np.uint32), pure.view(np.uint32))


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out_tensor(w, h, out_format=brt.FLAG_OUT_RGBA32F):
    import torch
    return torch.zeros((h, w * brt.OUT_PIXEL_BYTES[out_format] // 4), dtype=torch.int32, device="cuda")


def _host(t, h, w):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint8).reshape(h, w, -1)


class Raster:
    """The fixture at w x h on the device (rgba / depth None: a NULL pointer)."""

    def __init__(self, w, h, rgba="fixture", depth="fixture"):
        self.rgba = ubr.raster_rgba(w, h) if isinstance(rgba, str) else rgba
        self.depth = ubr.raster_depth(w, h) if isinstance(depth, str) else depth
        self.d_rgba = None if self.rgba is None else _device(self.rgba)
        self.d_depth = None if self.depth is None else _device(self.depth)

    def ptrs(self):
        return dict(d_raster_rgba=0 if self.d_rgba is None else self.d_rgba.data_ptr(),
                    d_raster_depth=0 if self.d_depth is None else self.d_depth.data_ptr())

    def texels(self, oracle, name, h, w):
        rgba = np.zeros((h, w, 4), F32) if self.rgba is None else self.rgba
        return _bits(rgba if name is None else oracle.encode_frame(rgba, name)).reshape(h, w, -1)


def _upscale(plugin, cam, win, lw, lh, d_low, w, h, out_format=brt.FLAG_OUT_RGBA32F, stream=None):
    out = _out_tensor(w, h, out_format)
    plugin.node.upscale_device(cam, win, lw, lh, d_low.data_ptr(), w, h, out.data_ptr(), stream=stream, out_format=out_format)
    return _host(out, h, w)


def _upscale_blend(plugin, level, cam, win, lw, lh, d_low, w, h, raster, out_format=brt.FLAG_OUT_RGBA32F, stream=None):
    out = _out_tensor(w, h, out_format)
    plugin.node.upscale_blend_device(level, cam, win, lw, lh, d_low.data_ptr(), w, h, out.data_ptr(), stream=stream, out_format=out_format,
                                     **raster.ptrs())
    return _host(out, h, w)


def _one_call(plugin, level, cam, win, lw, lh, w, h, raster, flags=0, out_format=brt.FLAG_OUT_RGBA32F, stream=None):
    out = _out_tensor(w, h, out_format)
    plugin.node.render_upscaled_blend_device(level, cam, win, lw, lh, w, h, out.data_ptr(), stream=stream, out_format=out_format,
                                             flags=flags, **raster.ptrs())
    return _host(out, h, w)


def _render_low(plugin, cam, win, lw, lh, h, spp=2, seed=None):
    """The Pure low frame of brt_render_device on the resident scene, on the device."""
    import torch
    low = torch.empty((lh, lw, 4), dtype=torch.float32, device="cuda")
    lvl3, _, _ = _view(lw, lh, spp)
    plugin.node.render_device(lvl3, cam, brt.upscale_window(win, h, lh), lw, lh, low.data_ptr())
    return low


def _upload(plugin, case):
    kind = brt.SCENE_STRESS_GRID if case == "stress" else brt.SCENE_COVER
    b = brt.generate_scene(kind, 1)
    plugin.node.write_buffers(b if case == "cover_caller" else brt.Buffers(b.models, b.materials, None))


def _where(cov, a, b):
    return np.where(cov[..., None], a, b)


EXACT_CASES = [("cover_callee", s) for s in SHAPES] + [("cover_caller", SHAPES[0]), ("stress", SHAPES[0])]


@pytest.mark.gpu
@pytest.mark.parametrize("case,shape", EXACT_CASES, ids=["%s-%dx%d_from_%dx%d" % ((c,) + s) for c, s in EXACT_CASES])
def test_covered_set_texels_and_uncovered_pixels_are_exact(plugin, oracle, case, shape):
    """At levels 1 and 2, in the four store formats: the covered set is brt_host_blend_covered of the t plane of
    brt_debug_denoise_guides at full size, a covered pixel is oracle.encode_frame of its texel, any other pixel is bit for bit
    brt_upscale_device's on the same low frame."""
    w, h, lw, lh = shape
    _upload(plugin, case)
    _, cam, win = _view(w, h)
    low = _render_low(plugin, cam, win, lw, lh, h)
    if case == "stress":
        assert plugin.node.last_stats["scene_in_lds"] == 2             # top of the tree in LDS, the rest from L2
    t = plugin.debug_denoise_guides(cam, win, w, h)[..., 3]
    raster = Raster(w, h)
    for level in (1, 2):
        lvl, _, _ = _view(w, h, level=level)
        cov = brt.blend_covered(cam, lvl, t, raster.depth)
        assert np.array_equal(cov, ubr.covered(cam, level, t, raster.depth))
        print(f"{case} {shape} level {level}: covered {ubr.class_shares(cov)[0]:.4f}")
        if w > 1:
            _assert_shares(cov)
            (ny, nx), (iy, ix) = ubr.special_texels(w, h)
            assert cov[ny, nx] and cov[iy, ix]
        for fmt, name in FORMATS:
            plain = _upscale(plugin, cam, win, lw, lh, low, w, h, out_format=fmt)
            got = _upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, raster, out_format=fmt)
            tex = raster.texels(oracle, name, h, w)
            assert np.array_equal(got[cov], tex[cov]), (level, name)
            assert np.array_equal(got[~cov], plain[~cov]), (level, name)
            # the covered SET: where texel and upsampled pixel differ, the output names its class
            differ = (tex != plain).any(-1)
            assert np.array_equal((got == tex).all(-1)[differ], cov[differ]), (level, name)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_frame_matches_the_restatement(plugin, oracle, shape):
    """The whole frame against upscale_blend_ref fed with the device's guides at both sizes, to section 14's 1e-4 max(1, |ref|); the
    sky and the covered pixels (NaN and Inf texels among them) bitwise.  Stage B occurs among the uncovered pixels at 96x54 (2 pixels)
    and at 161x91 (5), and is asserted there; 41x23 from 21x12 has no stage B pixel outside the raster's cover, so that case asserts
    stage A alone (tests/test_upscale_synthetic.py reaches stages B and C and the zero store under the blend)."""
    w, h, lw, lh = shape
    _upload(plugin, "cover_callee")
    _, cam, win = _view(w, h)
    low = _render_low(plugin, cam, win, lw, lh, h)
    g_low = plugin.debug_denoise_guides(cam, brt.upscale_window(win, h, lh), lw, lh)
    g_full = plugin.debug_denoise_guides(cam, win, w, h)
    raster = Raster(w, h)
    for level in (1, 2):
        lvl, _, _ = _view(w, h, level=level)
        got = _upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, raster).view(F32)
        want, stage = ubr.upscale_frame(oracle, low.cpu().numpy(), g_low, g_full, cam, level, raster.rgba, raster.depth)
        exact = (stage == ubr.COVERED) | (stage == ur.SKY)
        assert _same_bits(got[exact], want[exact]), level
        err = np.abs(got[~exact].astype(np.float64) - want[~exact]) / np.maximum(1.0, np.abs(want[~exact]))
        print(f"{shape} level {level}: max err {err.max() if err.size else 0.0:.3g}, stages {np.bincount(stage.ravel(), minlength=6).tolist()}")
        assert err.size == 0 or err.max() <= 1e-4, float(err.max())
        if w > 1:
            _assert_shares(stage == ubr.COVERED)
            assert (stage == ur.STAGE_A).any()
            if shape != (41, 23, 21, 12):
                assert (stage == ur.STAGE_B).any()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, brt.FLAG_DENOISE, brt.FLAG_TEMPORAL, brt.FLAG_DENOISE | brt.FLAG_TEMPORAL],
                         ids=["plain", "denoise", "temporal", "denoise_temporal"])
def test_one_call_equals_render_post_and_blend(plugin, flags):
    """render_upscaled_blend_device = render_device (Pure, low size) + denoise_device with the same flags + upscale_blend_device, bit
    for bit over 4 frames (the temporal history is that of the low size in both forms)."""
    import torch
    w, h, lw, lh = SHAPES[0]
    _upload(plugin, "cover_callee")
    raster = Raster(w, h)
    seeds = (0.5, 0.25, 0.75, 0.125)

    def sequence(one_call):
        plugin.reset_temporal()
        frames = []
        for seed in seeds:
            lvl, cam, win = _view(w, h, spp=4, level=2, seed=seed)
            if one_call:
                frames.append(_one_call(plugin, lvl, cam, win, lw, lh, w, h, raster, flags=flags))
                continue
            low = _render_low(plugin, cam, win, lw, lh, h, spp=4)
            if flags:
                post = torch.empty_like(low)
                plugin.node.denoise_device(cam, brt.upscale_window(win, h, lh), lw, lh, low.data_ptr(), post.data_ptr(), flags=flags)
                low = post
            frames.append(_upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, raster))
        return frames

    one, two = sequence(True), sequence(False)
    for k in range(len(seeds)):
        assert _same_bits(one[k], two[k]), k
    assert not _same_bits(one[0], one[1])
    plugin.reset_temporal()


@pytest.mark.gpu
def test_level_3_is_the_call_without_a_level(plugin):
    w, h, lw, lh = SHAPES[0]
    _upload(plugin, "cover_callee")
    lvl, cam, win = _view(w, h, spp=4, level=3)
    low = _render_low(plugin, cam, win, lw, lh, h, spp=4)
    raster = Raster(w, h)
    for fmt, _ in FORMATS:
        assert _same_bits(_upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, raster, out_format=fmt),
                          _upscale(plugin, cam, win, lw, lh, low, w, h, out_format=fmt))
        for flags in (0, brt.FLAG_DENOISE):
            out = _out_tensor(w, h, fmt)
            plugin.node.render_upscaled_device(cam, win, lw, lh, w, h, out.data_ptr(), out_format=fmt, flags=flags)
            assert _same_bits(_one_call(plugin, lvl, cam, win, lw, lh, w, h, raster, flags=flags, out_format=fmt), _host(out, h, w))
    # the raster inputs are not read at level 3: the output may be the raster colour's own memory
    plugin.node.upscale_blend_device(lvl, cam, win, lw, lh, low.data_ptr(), w, h, raster.d_rgba.data_ptr(), **raster.ptrs())
    assert _same_bits(_host(raster.d_rgba, h, w), _upscale(plugin, cam, win, lw, lh, low, w, h))


@pytest.mark.gpu
def test_edge_inputs(plugin):
    w, h, lw, lh = SHAPES[0]
    _upload(plugin, "cover_callee")
    _, cam, win = _view(w, h)
    low = _render_low(plugin, cam, win, lw, lh, h)
    pure = _upscale(plugin, cam, win, lw, lh, low, w, h)
    t = plugin.debug_denoise_guides(cam, win, w, h)[..., 3]
    sky = t == np.inf
    assert sky.any() and (t[~sky] <= F32(cam[0]["far"])).all()
    lvl1, lvl2 = _view(w, h, level=1)[0], _view(w, h, level=2)[0]
    fixture = Raster(w, h)
    tex = _bits(fixture.rgba).reshape(h, w, -1)
    # NULL depth: level 2 is the Pure upsampling, level 1 has exactly the sky pixels covered
    no_depth = Raster(w, h, depth=None)
    assert _same_bits(_upscale_blend(plugin, lvl2, cam, win, lw, lh, low, w, h, no_depth), pure)
    assert _same_bits(_upscale_blend(plugin, lvl1, cam, win, lw, lh, low, w, h, no_depth), _where(sky, tex, pure))
    # NULL colour: zero texels
    no_colour = Raster(w, h, rgba=None)
    for level, lvl in ((1, lvl1), (2, lvl2)):
        cov = ubr.covered(cam, level, t, fixture.depth)
        _assert_shares(cov)
        assert _same_bits(_upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, no_colour), _where(cov, np.zeros_like(pure), pure))
    both_null = Raster(w, h, rgba=None, depth=None)
    assert _same_bits(_upscale_blend(plugin, lvl1, cam, win, lw, lh, low, w, h, both_null), _where(sky, np.zeros_like(pure), pure))
    # a fully covered frame is the stored raster, whatever the low frame holds; a NaN depth never covers
    full = Raster(w, h, depth=np.full((h, w), 1.0e6, F32))
    assert ubr.covered(cam, 2, t, full.depth).all()
    import torch
    junk = torch.full((lh, lw, 4), float("nan"), dtype=torch.float32, device="cuda")
    for lvl in (lvl1, lvl2):
        assert _same_bits(_upscale_blend(plugin, lvl, cam, win, lw, lh, junk, w, h, full), tex)
        assert _same_bits(_one_call(plugin, lvl, cam, win, lw, lh, w, h, full), tex)
    nan_depth = Raster(w, h, depth=np.full((h, w), np.nan, F32))
    for lvl in (lvl1, lvl2):
        assert _same_bits(_upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, nan_depth), pure)


@pytest.mark.gpu
def test_other_paths_are_unchanged_between_blended_calls(plugin):
    """Plain brt_upscale_device / brt_render_upscaled_device frames and plain level-2 brt_render_device frames rendered between
    blended calls are what they were before."""
    import torch
    w, h, lw, lh = SHAPES[0]
    _upload(plugin, "cover_callee")
    lvl2, cam, win = _view(w, h, spp=4, level=2)
    raster = Raster(w, h)
    low = _render_low(plugin, cam, win, lw, lh, h, spp=4)
    frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")

    def others():
        a = _upscale(plugin, cam, win, lw, lh, low, w, h)
        out = _out_tensor(w, h)
        plugin.node.render_upscaled_device(cam, win, lw, lh, w, h, out.data_ptr(), flags=brt.FLAG_DENOISE)
        plugin.node.render_device(lvl2, cam, win, w, h, frame.data_ptr(), **raster.ptrs())
        return a, _host(out, h, w), frame.cpu().numpy()

    def blended():
        _upscale_blend(plugin, lvl2, cam, win, lw, lh, low, w, h, raster)
        _one_call(plugin, lvl2, cam, win, lw, lh, w, h, raster, flags=brt.FLAG_DENOISE)
        _one_call(plugin, _view(w, h, level=1)[0], cam, win, lw, lh, w, h, raster, out_format=brt.FLAG_OUT_RGBA16F)

    before = others()
    blended()
    between = others()
    blended()
    after = others()
    for k in range(3):
        assert _same_bits(before[k], between[k]) and _same_bits(before[k], after[k]), k
    assert (before[2][..., 3] != 1).any()                              # (the level-2 frame did blend: the raster's alpha shows)


@pytest.mark.gpu
def test_streams(plugin):
    """A caller's stream, and two calls of each form in flight on two streams: every result is the synchronous call's."""
    import torch
    w, h, lw, lh = SHAPES[0]
    _upload(plugin, "cover_callee")
    raster = Raster(w, h)
    views = [_view(w, h, spp=4, level=2, seed=s) for s in (0.5, 0.25)]
    lows = [_render_low(plugin, cam, win, lw, lh, h, spp=4) for _, cam, win in views]
    want_up = [_upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, raster) for (lvl, cam, win), low in zip(views, lows)]
    want_one = [_one_call(plugin, lvl, cam, win, lw, lh, w, h, raster, flags=brt.FLAG_DENOISE) for lvl, cam, win in views]
    assert not _same_bits(want_one[0], want_one[1])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    node, ptrs = plugin.node, raster.ptrs()
    outs = [_out_tensor(w, h) for _ in range(2)]
    lvl, cam, win = views[0]
    node.upscale_blend_device(lvl, cam, win, lw, lh, lows[0].data_ptr(), w, h, outs[0].data_ptr(), stream=s1.cuda_stream, **ptrs)
    node.render_upscaled_blend_device(lvl, cam, win, lw, lh, w, h, outs[1].data_ptr(), stream=s1.cuda_stream, flags=brt.FLAG_DENOISE, **ptrs)
    s1.synchronize()
    assert _same_bits(_host(outs[0], h, w), want_up[0]) and _same_bits(_host(outs[1], h, w), want_one[0])
    outs = [_out_tensor(w, h) for _ in range(8)]
    for r in range(2):
        for k, s in enumerate((s1, s2)):
            lvl, cam, win = views[k]
            node.render_upscaled_blend_device(lvl, cam, win, lw, lh, w, h, outs[4 * r + k].data_ptr(), stream=s.cuda_stream,
                                              flags=brt.FLAG_DENOISE, **ptrs)
            node.upscale_blend_device(lvl, cam, win, lw, lh, lows[k].data_ptr(), w, h, outs[4 * r + 2 + k].data_ptr(), stream=s.cuda_stream,
                                      **ptrs)
    s1.synchronize()
    s2.synchronize()
    for r in range(2):
        for k in range(2):
            assert _same_bits(_host(outs[4 * r + k], h, w), want_one[k]), (r, k)
            assert _same_bits(_host(outs[4 * r + 2 + k], h, w), want_up[k]), (r, k)


@pytest.mark.gpu
def test_refusals(plugin):
    import torch
    w, h, lw, lh = 64, 40, 32, 20
    _upload(plugin, "cover_callee")
    lvl, cam, win = _view(w, h, level=2)
    low = _render_low(plugin, cam, win, lw, lh, h)
    raster = Raster(w, h)
    buf = torch.zeros((2 * h + lh, w, 4), dtype=torch.float32, device="cuda")
    out = buf[:h]
    before = _upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, raster)
    lib, ctx, c, wn = plugin._lib, plugin._ctx, cam.ctypes.data, win.ctypes.data
    rr, rd = raster.d_rgba.data_ptr(), raster.d_depth.data_ptr()

    def up(level=2, lw_=lw, lh_=lh, w_=w, h_=h, d_low=low.data_ptr(), d_out=out.data_ptr(), flags=0, cam_=c, win_=wn, rr_=rr, rd_=rd):
        return lib.brt_upscale_blend_device(ctx, cam_, win_, level, lw_, lh_, d_low, w_, h_, rr_, rd_, d_out, None, flags, None)

    def one(level=2, lw_=lw, lh_=lh, w_=w, h_=h, d_out=out.data_ptr(), flags=0, cam_=c, win_=wn, rr_=rr, rd_=rd):
        return lib.brt_render_upscaled_blend_device(ctx, cam_, win_, level, lw_, lh_, w_, h_, rr_, rd_, d_out, None, flags, None)

    assert up() == 0 and one() == 0 and up(level=1) == 0 and one(level=1) == 0 and up(level=3) == 0 and one(level=3) == 0
    whole = buf.data_ptr()
    for call in (up, one):
        assert call(level=0) == ERR_UNSUPPORTED
        for level in (4, 5, 1 << 31, 0xFFFFFFFF):
            assert call(level=level) == ERR_INVALID, (call.__name__, level)
        for sizes in (dict(lw_=0), dict(lh_=0), dict(lw_=w + 1), dict(lh_=h + 1), dict(w_=4 * lw + 1), dict(h_=4 * lh + 1),
                      dict(lw_=16384, lh_=lh, w_=32769, h_=h), dict(lw_=lw, lh_=16384, w_=w, h_=32769)):
            assert call(**sizes) == ERR_INVALID, (call.__name__, sizes)
        for flags in (brt.FLAG_COUNTERS, brt.FLAG_KERNEL_SIMPLE, brt.FLAG_BLEND_POST, 256, 1 << 31):
            assert call(flags=flags) == ERR_INVALID, (call.__name__, flags)
        assert call(d_out=None) == ERR_INVALID and call(cam_=None) == ERR_INVALID and call(win_=None) == ERR_INVALID
        # the output must overlap neither raster buffer (levels 1 / 2)
        for level in (1, 2):
            assert call(level=level, d_out=whole, rr_=whole) == ERR_INVALID
            assert call(level=level, d_out=whole, rr_=whole + (w * h - 1) * 16) == ERR_INVALID
            assert call(level=level, d_out=whole + (w * h - 1) * 16, rr_=whole) == ERR_INVALID
            assert call(level=level, d_out=whole, rd_=whole) == ERR_INVALID
            assert call(level=level, d_out=whole, rd_=whole + w * h * 16 - 4) == ERR_INVALID
            assert call(level=level, d_out=whole + (w * h - 1) * 4, rd_=whole) == ERR_INVALID
        assert call(d_out=whole, rr_=whole + w * h * 16) == 0                                         # adjacent: fine
    for flags in (brt.FLAG_DENOISE, brt.FLAG_TEMPORAL):                # the post-passes belong to the one-call form
        assert up(flags=flags) == ERR_INVALID
        assert one(flags=flags) == 0
    plugin.reset_temporal()
    assert up(d_low=None) == ERR_INVALID
    # d_out must not overlap d_low_rgba
    low_at = whole + 2 * w * h * 16
    assert up(d_low=whole, d_out=whole) == ERR_INVALID
    assert up(d_low=whole + (w * h - 1) * 16, d_out=whole) == ERR_INVALID
    assert up(d_low=whole, d_out=whole + (lw * lh - 1) * 16) == ERR_INVALID
    assert up(d_low=low_at, d_out=whole) == 0
    # before any upload
    with brt.RaytracePlugin([0]) as fresh:
        assert fresh._lib.brt_upscale_blend_device(fresh._ctx, c, wn, 2, lw, lh, low.data_ptr(), w, h, rr, rd, out.data_ptr(), None, 0,
                                                   None) == ERR_NO_SCENE
        assert fresh._lib.brt_render_upscaled_blend_device(fresh._ctx, c, wn, 2, lw, lh, w, h, rr, rd, out.data_ptr(), None, 0,
                                                           None) == ERR_NO_SCENE
    # the context is as usable as before
    assert _same_bits(_upscale_blend(plugin, lvl, cam, win, lw, lh, low, w, h, raster), before)
