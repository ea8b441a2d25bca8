"""The guide-buffer a-trous denoiser (BRT_FLAG_DENOISE, brt_denoise_device, brt_set_denoise, brt_debug_denoise_guides; DESIGN.md
"Denoiser").  CPU: the exports, the argument checks, properties of the numpy restatement (tests/denoise_ref.py) and its quality bar.
GPU: guides bitwise against the oracle's raycast, the filter against the restatement, the store formats, the three entry points, no
change to frames rendered without the flag, quality, rejections."""
import numpy as np
import pytest

import bevyray_amd as brt
from bevyray_amd import _lib
import denoise_ref as dr
from helpers import uniforms

F32 = np.float32
ERR_INVALID, ERR_NO_SCENE, ERR_UNSUPPORTED = -1, -7, -8
# Quality bars: MSE of the denoised frame over the hit pixels, relative to the noisy one's, both against a 1024-spp frame of another
# seed, cover scene, 8 bounces (quality).  {spp: bar}.  CPU restatement at 96x54: measured 0.773 at 4 spp,
# 0.951 at 64 spp (above 4 spp the strength falls with the noise std, so the filter does not trade noise for more bias).  GPU at
# 480x270, set from its own measurement: 0.305 at 4 spp, 0.858 at 64 spp (the frames and the filter are deterministic).
CPU_BARS = {4: 0.85, 64: 0.97}
GPU_BARS = {4: 0.40, 64: 0.90}


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_denoise_exports_exist():
    lib = _lib.load()
    for name in ("brt_set_denoise", "brt_denoise_device", "brt_debug_denoise_guides"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert brt.FLAG_DENOISE == 32 and lib.brt_abi_version() == 6


def test_denoise_argument_checks_without_a_context():
    lib = _lib.load()
    cam, win = np.zeros(80, np.uint8), np.zeros(16, np.uint8)
    assert lib.brt_set_denoise(None, 5, 4.0, 128.0, 1.0) == ERR_INVALID
    assert lib.brt_denoise_device(None, cam.ctypes.data, win.ctypes.data, 8, 8, 16, 16, None, 0, None) == ERR_INVALID
    out = np.zeros(8 * 8 * 8, F32)
    assert lib.brt_debug_denoise_guides(None, cam.ctypes.data, win.ctypes.data, 8, 8, out.ctypes.data) == ERR_INVALID


def _flat_guides(h, w, n=(0.0, 0.0, 1.0), t=5.0, a=(0.5, 0.6, 0.7)):
    g = np.zeros((h, w, 8), F32)
    g[..., 0:3] = n
    g[..., 3] = t
    g[..., 4:7] = a
    g[..., 7] = 0
    dirs = np.zeros((h, w, 3), F32)
    dirs[..., 2] = -1
    return g, dirs


def test_restatement_keeps_a_constant_image():
    h, w = 24, 40
    g, dirs = _flat_guides(h, w)
    frame = np.empty((h, w, 4), F32)
    frame[...] = (0.3, 0.45, 0.6, 1.0)
    for it in (1, 5, 6):
        out = dr.denoise(frame, g, dirs, 0.2, iterations=it)
        assert np.abs(out - frame).max() <= 1e-6


def test_restatement_does_not_blur_across_a_normal_step():
    """Two spheres side by side whose normals differ by more than 90 degrees: w_n = 0 across the step."""
    h, w = 20, 32
    g, dirs = _flat_guides(h, w)
    g[:, w // 2:, 0:3] = (0.8, 0.0, -0.6)          # n_left . n_right = -0.6
    rng = np.random.default_rng(1)
    frame = np.ones((h, w, 4), F32)
    frame[:, : w // 2, :3] = 0.2 + 0.05 * rng.standard_normal((h, w // 2, 3)).astype(F32)
    frame[:, w // 2:, :3] = 0.8 + 0.05 * rng.standard_normal((h, w - w // 2, 3)).astype(F32)
    out = dr.denoise(frame, g, dirs, 0.2)
    left, right = out[:, : w // 2, :3], out[:, w // 2:, :3]
    # no colour crosses the step: every output is a weighted mean of its own side's inputs only
    for got, src in ((left, frame[:, : w // 2, :3]), (right, frame[:, w // 2:, :3])):
        assert (got >= src.min(axis=(0, 1)) - 1e-6).all() and (got <= src.max(axis=(0, 1)) + 1e-6).all()


def test_restatement_passes_sky_and_non_finite_pixels_through():
    h, w = 24, 24
    g, dirs = _flat_guides(h, w)
    rng = np.random.default_rng(2)
    frame = np.ones((h, w, 4), F32)
    frame[..., :3] = 0.4 + 0.1 * rng.standard_normal((h, w, 3)).astype(F32)
    frame[..., 3] = 0.75
    sky = np.zeros((h, w), bool)
    sky[:6, :] = True
    sky[10, 10] = True
    g[sky, 3] = np.inf
    g[sky, 0:3] = 0
    g[sky, 4:7] = 1
    bad = [(15, 3), (20, 20)]
    a = frame.copy()
    a[sky, :3] = (0.9, 0.95, 1.0)
    a[15, 3, 0], a[20, 20, 2] = np.nan, np.inf
    b = a.copy()
    b[sky, :3] = (5.0, -3.0, 7.0)                   # other sky colours, other non-finite values
    b[15, 3, 0], b[20, 20, 2] = -np.inf, np.nan
    out_a, out_b = dr.denoise(a, g, dirs, 0.2), dr.denoise(b, g, dirs, 0.2)
    through = sky.copy()
    for y, x in bad:
        through[y, x] = True
    assert np.array_equal(out_a[through].view(np.uint32), a[through].view(np.uint32))
    assert np.array_equal(out_b[through].view(np.uint32), b[through].view(np.uint32))
    # ... and they spread into no neighbour: the other pixels are the same bits whatever those pixels hold
    assert np.isfinite(out_a[~through]).all()
    assert np.array_equal(out_a[~through].view(np.uint32), out_b[~through].view(np.uint32))


@pytest.mark.parametrize("spp", [4, 64])
def test_restatement_quality_bar(oracle, spp):
    """The cover scene at 96x54: the denoised frame has at most CPU_BARS[spp] x the noisy frame's MSE against 1024 spp."""
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 96, 54
    lvl, cam, win = brt.cover_camera(w, h, spp, 8, brt.Raytracing.Pure, 0.5)
    noisy, _ = oracle.render(b, lvl, cam, win, w, h)
    lvl_r, cam_r, win_r = brt.cover_camera(w, h, 1024, 8, brt.Raytracing.Pure, 0.25)
    ref, _ = oracle.render(b, lvl_r, cam_r, win_r, w, h)
    g = dr.guides(oracle, b, cam, w, h)
    assert (g[..., 3] < np.inf).sum() > w * h // 2
    out = dr.denoise_frame(oracle, noisy, g, cam)
    ratio = dr.hit_mse(out, ref, g) / dr.hit_mse(noisy, ref, g)
    assert ratio <= CPU_BARS[spp], ratio


def test_restatement_strength_follows_the_sample_count():
    """Above 4 spp sigma_l and the blend weight scale by sqrt(4 / spp): a frame rendered at 16 spp moves half as far as at 4 spp
    (with sigma_l off the table: a constant luminance, so w_l = 1 at any scale)."""
    assert dr.strength(1) == dr.strength(4) == 1 and dr.strength(16) == F32(0.5) and dr.strength(64) == F32(0.25)
    h, w = 16, 16
    g, dirs = _flat_guides(h, w, a=(1.0, 1.0, 1.0))
    frame = np.ones((h, w, 4), F32)
    frame[..., :3] = 0.4
    frame[::2, :, 0] = 0.6                                  # stripes of another colour with the same luminance
    frame[::2, :, 1] = 0.4 - (0.6 - 0.4) * 0.2126 / 0.7152
    d4, d16 = dr.denoise(frame, g, dirs, 0.2, spp=4), dr.denoise(frame, g, dirs, 0.2, spp=16)
    assert np.abs((d16 - frame) - 0.5 * (d4 - frame)).max() <= 1e-5


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _denoise_dev(plugin, cam, win, w, h, frame, out_format=brt.FLAG_OUT_RGBA32F, stream=None):
    import torch
    d_in = _device(frame)
    out = torch.zeros((h, w * brt.OUT_PIXEL_BYTES[out_format] // 4), dtype=torch.int32, device="cuda")
    plugin.node.denoise_device(cam, win, w, h, d_in.data_ptr(), out.data_ptr(), stream=stream, out_format=out_format)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint8).reshape(h, w, -1)


def _assert_guides_equal(got, want):
    assert got.shape == want.shape
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{bad.sum()} pixels differ, first {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cover_callee", "cover_caller", "rtiow", "stress", "far"])
def test_guides_match_the_oracle_raycast(plugin, oracle, case):
    w, h = 320, 180
    kind = {"rtiow": brt.SCENE_RTIOW_FINAL, "stress": brt.SCENE_STRESS_GRID}.get(case, brt.SCENE_COVER)
    b = brt.generate_scene(kind, 1)
    if case == "stress":
        w, h = 160, 90
    if case == "far":
        w, h = 160, 90
        lvl, cam, win = uniforms(w, h, 2, 4, (13.0 * 20, 2.0 * 20, 3.0 * 20), (0.0, 0.0, 0.0), 0.4 / 20, 0.5, far=1.0e5)
    elif case == "rtiow":
        lvl, cam, win = brt.rtiow_camera(w, h, 2, 4)
    else:
        lvl, cam, win = brt.cover_camera(w, h, 2, 4)
    if case in ("cover_callee", "far"):
        plugin.node.run(lvl, cam, win, w, h, buffers=brt.Buffers(b.models, b.materials, None))
        st = plugin.node.last_stats
        tree = brt.build_bvh_sah(b.models, st["tree_reach"])        # the CPU twin of the tree the context walks
    else:
        plugin.node.run(lvl, cam, win, w, h, buffers=b)
        st = plugin.node.last_stats
        tree = b.bvh
    if case == "stress":
        assert st["scene_in_lds"] == 2                               # top of the tree in LDS, the rest from L2
    got = plugin.debug_denoise_guides(cam, win, w, h)
    want = dr.guides(oracle, brt.Buffers(b.models, b.materials, tree), cam, w, h)
    _assert_guides_equal(got, want)
    assert (got[..., 3] < np.inf).any()


@pytest.fixture
def cover_noisy(plugin):
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 640, 360
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, 0.5)
    frame = plugin.node.run(lvl, cam, win, w, h, buffers=b).copy()
    g = plugin.debug_denoise_guides(cam, win, w, h)
    yield b, lvl, cam, win, w, h, frame, g
    plugin.set_denoise()


@pytest.mark.gpu
def test_filter_matches_the_restatement(plugin, oracle, cover_noisy):
    _, _, cam, win, w, h, frame, g = cover_noisy
    _, dirs, scale = dr.pixel_center_rays(oracle, cam, w, h)
    settings = [dict(iterations=i) for i in (1, 2, 3, 4, 5)] + [dict(iterations=3, sigma_l=2.5, sigma_n=32.0, sigma_z=0.5)]
    for s in settings:
        full = {**dr.DEFAULTS, **s}
        plugin.set_denoise(full["iterations"], full["sigma_l"], full["sigma_n"], full["sigma_z"])
        got = _denoise_dev(plugin, cam, win, w, h, frame).view(F32)
        want = dr.denoise(frame, g, dirs, scale, spp=4, **full)
        err = np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
        assert err.max() <= 1e-4, (s, float(err.max()))
        assert np.abs(got - frame).max() > 1e-3                       # (it did filter)
    # a 16-spp frame: sigma_l and the blend weight at half strength
    plugin.set_denoise()
    lvl16, cam16, win16 = brt.cover_camera(w, h, 16, 8, brt.Raytracing.Pure, 0.5)
    f16 = plugin.node.run(lvl16, cam16, win16, w, h).copy()
    got = _denoise_dev(plugin, cam16, win16, w, h, f16).view(F32)
    want = dr.denoise(f16, g, dirs, scale, spp=16, **dr.DEFAULTS)
    err = np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-4, float(err.max())


@pytest.mark.gpu
def test_output_formats_are_the_store_of_the_f32_result(plugin, oracle, cover_noisy):
    _, _, cam, win, w, h, frame, _ = cover_noisy
    f32 = _denoise_dev(plugin, cam, win, w, h, frame).view(F32)
    for fmt, name in ((brt.FLAG_OUT_RGBA8_UNORM_SRGB, "srgb8"), (brt.FLAG_OUT_RGBA8_UNORM, "unorm8"), (brt.FLAG_OUT_RGBA16F, "f16")):
        got = _denoise_dev(plugin, cam, win, w, h, frame, out_format=fmt)
        want = oracle.encode_frame(f32, name)
        assert np.array_equal(got.view(want.dtype).reshape(want.shape), want), name


@pytest.mark.gpu
def test_entry_points_agree_and_leave_plain_frames_alone(plugin, oracle):
    import torch
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 200, 120
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, 0.5)
    want, _ = oracle.render(b, lvl, cam, win, w, h)
    plain = plugin.node.run(lvl, cam, win, w, h, buffers=b).copy()
    assert np.array_equal(plain.view(np.uint32), want.view(np.uint32))
    via_run = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE).copy()
    assert not np.array_equal(via_run, plain)
    again = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE).copy()
    assert np.array_equal(again.view(np.uint32), via_run.view(np.uint32))             # deterministic
    frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    plugin.node.render_device(lvl, cam, win, w, h, frame.data_ptr(), flags=brt.FLAG_DENOISE)
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), via_run.view(np.uint32))
    plugin.node.render_device(lvl, cam, win, w, h, frame.data_ptr())
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), want.view(np.uint32))
    out = torch.empty_like(frame)
    plugin.node.denoise_device(cam, win, w, h, frame.data_ptr(), out.data_ptr())
    assert np.array_equal(out.cpu().numpy().view(np.uint32), via_run.view(np.uint32))
    plugin.node.denoise_device(cam, win, w, h, frame.data_ptr(), frame.data_ptr())    # in place
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), via_run.view(np.uint32))
    # the caller's stream (BRT_FLAG_CALLER_STREAM), asynchronous
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        f2, o2 = torch.empty_like(frame), torch.empty_like(frame)
        plugin.node.render_device(lvl, cam, win, w, h, f2.data_ptr(), stream=s.cuda_stream, flags=brt.FLAG_DENOISE)
        plugin.node.render_device(lvl, cam, win, w, h, o2.data_ptr(), stream=s.cuda_stream)
        plugin.node.denoise_device(cam, win, w, h, o2.data_ptr(), o2.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(f2.cpu().numpy().view(np.uint32), via_run.view(np.uint32))
    assert np.array_equal(o2.cpu().numpy().view(np.uint32), via_run.view(np.uint32))
    # and after all of it a plain frame is still the oracle's (scratch, settings and dispatch-order history disturb nothing)
    after = plugin.node.run(lvl, cam, win, w, h)
    assert np.array_equal(after.view(np.uint32), want.view(np.uint32))
    plugin.node.render_device(lvl, cam, win, w, h, frame.data_ptr())
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [4, 64])
def test_quality_on_the_gpu(plugin, spp):
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 480, 270
    _, cam_r, win_r = brt.cover_camera(w, h, 1024, 8, brt.Raytracing.Pure, 0.25)
    lvl, cam, win = brt.cover_camera(w, h, spp, 8, brt.Raytracing.Pure, 0.5)
    ref = plugin.node.run(lvl, cam_r, win_r, w, h, buffers=b).copy()
    noisy = plugin.node.run(lvl, cam, win, w, h).copy()
    den = plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE).copy()
    g = plugin.debug_denoise_guides(cam, win, w, h)
    ratio = dr.hit_mse(den, ref, g) / dr.hit_mse(noisy, ref, g)
    print(f"quality at {spp} spp: {ratio:.3f}")
    assert ratio <= GPU_BARS[spp], ratio


@pytest.mark.gpu
def test_rejections(plugin):
    import torch
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 64, 40
    plugin.node.write_buffers(b)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    for level in (brt.Raytracing.Skip, brt.Raytracing.FallbackRaster, brt.Raytracing.FallbackRaytraced):
        lvl, cam, win = brt.cover_camera(w, h, 2, 4, level)
        with pytest.raises(brt.BrtError) as e:
            plugin.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE)
        assert e.value.code == ERR_UNSUPPORTED
        with pytest.raises(brt.BrtError) as e:
            plugin.node.render_device(lvl, cam, win, w, h, frame.data_ptr(), flags=brt.FLAG_DENOISE)
        assert e.value.code == ERR_UNSUPPORTED
    lvl, cam, win = brt.cover_camera(w, h, 2, 4)
    with pytest.raises(brt.BrtError) as e:
        plugin.node.render_part_device(lvl, cam, win, w, h, 0, 1, frame.data_ptr(), flags=brt.FLAG_DENOISE)
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(brt.BrtError) as e:
        plugin.node.deinterleave_device(frame.data_ptr(), 1, w, h, frame.data_ptr(), out_format=brt.FLAG_DENOISE)
    assert e.value.code == ERR_UNSUPPORTED
    # invalid settings are refused and change nothing
    src = plugin.node.run(lvl, cam, win, w, h).copy()
    plugin.set_denoise(3, 2.0, 64.0, 0.5)
    before = _denoise_dev(plugin, cam, win, w, h, src)
    for args in ((0, 4.0, 128.0, 1.0), (7, 4.0, 128.0, 1.0), (5, 0.0, 128.0, 1.0), (5, 4.0, -1.0, 1.0), (5, 4.0, 128.0, float("nan")),
                 (5, float("inf"), 128.0, 1.0)):
        with pytest.raises(brt.BrtError) as e:
            plugin.set_denoise(*args)
        assert e.value.code == ERR_INVALID
    assert np.array_equal(_denoise_dev(plugin, cam, win, w, h, src), before)
    plugin.set_denoise()
    d_src = _device(src)
    assert plugin._lib.brt_denoise_device(plugin._ctx, cam.ctypes.data, win.ctypes.data, w, h, d_src.data_ptr(), d_src.data_ptr(), None,
                                          brt.FLAG_COUNTERS, None) == ERR_INVALID
    # before any upload
    with brt.RaytracePlugin([0]) as fresh:
        with pytest.raises(brt.BrtError) as e:
            _denoise_dev(fresh, cam, win, w, h, src)
        assert e.value.code == ERR_NO_SCENE
