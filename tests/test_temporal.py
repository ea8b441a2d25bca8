"""Temporal reprojection and accumulation (BRT_FLAG_TEMPORAL, brt_set_temporal, brt_reset_temporal, brt_debug_temporal_state;
DESIGN.md section 11).  CPU: the exports, the argument checks, properties of the numpy restatement (tests/temporal_ref.py) and its
quality bar.  GPU: a first frame equals the frame without the flag, still frames accumulate to the mean, reprojection and output
against the restatement (camera orbit, a moving sphere), lifecycle, entry points, rejections and quality."""
import numpy as np
import pytest

import bevyray_amd as brt
from bevyray_amd import _lib
import denoise_ref as dr
import temporal_ref as tr
from helpers import uniforms

F32 = np.float32
ERR_INVALID, ERR_UNSUPPORTED = -1, -8
FORMATS = (brt.FLAG_OUT_RGBA32F, brt.FLAG_OUT_RGBA8_UNORM_SRGB, brt.FLAG_OUT_RGBA16F, brt.FLAG_OUT_RGBA8_UNORM)
# Quality bars: MSE over the hit pixels against a 1024-spp frame of another seed, of the last of 8 FLAG_TEMPORAL | FLAG_DENOISE frames
# relative to one FLAG_DENOISE frame (quality).  CPU restatement at 96x54, 4 spp, still camera: measured 0.149.
# GPU at 480x270, set from its own measurement (the frames and the filters are deterministic): still camera 0.286 at 4 spp and 0.197 at
# 64 spp, a slow orbit (0.25 degrees per frame) 0.932 at 4 spp.
CPU_BAR = 0.25
GPU_BARS = {"still4": 0.33, "still64": 0.23, "orbit4": 0.97}


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_temporal_exports_exist():
    lib = _lib.load()
    for name in ("brt_set_temporal", "brt_reset_temporal", "brt_debug_temporal_state"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert brt.FLAG_TEMPORAL == 64 and lib.brt_abi_version() == 6


def test_temporal_argument_checks_without_a_context():
    lib = _lib.load()
    for m in (0, 1, 32, 65535, 65536):
        assert lib.brt_set_temporal(None, m) == ERR_INVALID
    assert lib.brt_reset_temporal(None) == ERR_INVALID
    out = np.zeros(8 * 8 * 8, F32)
    assert lib.brt_debug_temporal_state(None, 8, 8, out.ctypes.data) == ERR_INVALID


def _plane(w=48, h=32, o=(0.0, 0.0, 0.0), depth=10.0, tan=0.2):
    """A camera looking down -z at the plane z = -depth (normal +z, one sphere, one material) and its guides."""
    cam = tr.Camera.synthetic(o, (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), tan, w, h)
    g = np.zeros((h, w, 8), F32)
    g[..., 2] = 1.0
    g[..., 3] = ((F32(o[2]) + F32(depth)) / -cam.dirs[..., 2]).astype(F32)
    g[..., 4:7] = (0.5, 0.6, 0.7)
    sid = np.zeros((h, w), np.uint32)
    return cam, g, sid


def _noisy(rng, h, w, base=0.4):
    f = np.ones((h, w, 4), F32)
    f[..., :3] = base + 0.1 * rng.standard_normal((h, w, 3)).astype(F32)
    return f


SPHERES = np.array([[0.0, 0.0, -1000.0, 1.0e6]], F32)


def test_restatement_first_frame_is_the_frame_without_the_flag():
    """(a): an empty history gives the plain frame (FLAG_TEMPORAL alone) and the FLAG_DENOISE frame (with FLAG_DENOISE) bit for bit."""
    cam, g, sid = _plane()
    g[:4, :, 3] = np.inf                                  # some sky
    frame = _noisy(np.random.default_rng(1), *g.shape[:2])
    frame[10, 10, 0] = np.nan                             # and a non-finite pixel
    for spp in (4, 64):
        out = tr.frame_step(tr.History(), frame, g, sid, cam, SPHERES, spp, False)
        assert np.array_equal(out.view(np.uint32), frame.view(np.uint32))
        out = tr.frame_step(tr.History(), frame, g, sid, cam, SPHERES, spp, True)
        want = dr.denoise(frame, g, cam.dirs, cam.tan, spp=spp, **dr.DEFAULTS)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_restatement_still_frames_are_the_running_mean():
    """(b): K still frames with max_history >= K accumulate to the mean of the K demodulated inputs, n = K, identity reprojection."""
    cam, g, sid = _plane()
    rng = np.random.default_rng(2)
    hist = tr.History(max_history=8)
    frames = [_noisy(rng, *g.shape[:2]) for _ in range(8)]
    for f in frames:
        hp, _, _ = tr.accumulate(hist, f, g, sid, cam, SPHERES)
    mean = np.mean([f[..., :3].astype(np.float64) / g[..., 4:7] for f in frames], axis=0)
    assert np.abs(hp[..., :3] - mean).max() <= 1e-5 * np.abs(mean).max()
    st = tr.state(hist)
    assert (st[..., 3] == 8).all()
    gy, gx = np.mgrid[0:g.shape[0], 0:g.shape[1]]
    assert np.array_equal(st[..., 6], gx.astype(F32)) and np.array_equal(st[..., 7], gy.astype(F32))
    # one more frame: n stays at max_history, alpha = 1 / 8
    hp, _, _ = tr.accumulate(hist, frames[0], g, sid, cam, SPHERES)
    assert (hp[..., 3] == 8).all()


@pytest.mark.parametrize("shift", [(3, 0), (-2, 1), (0, -4)])
def test_restatement_translation_by_whole_pixels(shift):
    """A camera translated by whole pixels parallel to a plane: x', y' move by that many pixels, the history moves with them, and the
    revealed band starts again at n = 1."""
    w, h, depth, tan = 48, 32, 10.0, 0.2
    px = 2.0 * tan * depth / h                            # the world size of one pixel on the plane
    kx, ky = shift
    cam0, g0, sid = _plane(w, h, depth=depth, tan=tan)
    # the second camera sits kx pixels to the right / ky pixels down of the first: the point at pixel p was at p + (kx, -ky) before
    cam1, g1, _ = _plane(w, h, o=(kx * px, -ky * px, 0.0), depth=depth, tan=tan)
    rng = np.random.default_rng(3)
    f0, f1 = _noisy(rng, h, w), _noisy(rng, h, w)
    hist = tr.History()
    hp0, _, _ = tr.accumulate(hist, f0, g0, sid, cam0, SPHERES)
    hp1, _, _ = tr.accumulate(hist, f1, g1, sid, cam1, SPHERES)
    st = tr.state(hist)
    gy, gx = np.mgrid[0:h, 0:w]
    sx, sy = gx + kx, gy + ky
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    kept = st[..., 3] == 2
    assert kept[inside].all()
    # (a source a rounding error past the edge still has one tap inside, at a weight of that rounding error)
    extra = kept & ~inside
    assert ((sx[extra] >= -1) & (sx[extra] <= w) & (sy[extra] >= -1) & (sy[extra] <= h)).all()
    inside = kept
    assert np.abs(st[..., 6][inside] - sx[inside]).max() <= 1e-3
    assert np.abs(st[..., 7][inside] - sy[inside]).max() <= 1e-3
    assert (st[..., 3][~inside] == 1).all() and np.isnan(st[..., 6][~inside]).all()
    sxc, syc = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    want = 0.5 * (hp0[..., :3][syc[inside], sxc[inside]] + (f1[..., :3] / g1[..., 4:7])[inside])
    assert np.abs(hp1[..., :3][inside] - want).max() <= 1e-3    # (bilinear weights of an almost-integer position)


def test_restatement_rejects_other_surfaces():
    """A tap on another sphere, another material, a turned normal or another distance is not history."""
    cam, g, sid = _plane()
    rng = np.random.default_rng(4)
    hist = tr.History()
    tr.accumulate(hist, _noisy(rng, *g.shape[:2]), g, sid, cam, SPHERES)
    g2, sid2 = g.copy(), sid.copy()
    sid2[0:4] = 1
    g2[4:8, :, 7] = np.array([3], np.uint32).view(F32)[0]
    g2[8:12, :, 0:3] = (0.6, 0.0, 0.8)
    g2[12:16, :, 3] *= F32(1.5)
    hp, _, _ = tr.accumulate(hist, _noisy(rng, *g.shape[:2]), g2, sid2, cam, np.concatenate([SPHERES, SPHERES]))
    assert (hp[0:16, :, 3] == 1).all() and (hp[16:, :, 3] == 2).all()


def test_restatement_max_history_one_is_the_single_frame_denoise():
    cam, g, sid = _plane()
    rng = np.random.default_rng(5)
    hist = tr.History(max_history=1)
    for _ in range(3):
        f = _noisy(rng, *g.shape[:2])
        out = tr.frame_step(hist, f, g, sid, cam, SPHERES, 4, True)
        want = dr.denoise(f, g, cam.dirs, cam.tan, spp=4, **dr.DEFAULTS)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def _seed(i):
    return 0.5 + 0.0371 * i


def test_restatement_quality_bar(oracle):
    """The cover scene at 96x54: 8 still frames of 4 spp, FLAG_TEMPORAL | FLAG_DENOISE, against one FLAG_DENOISE frame."""
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 96, 54
    lvl_r, cam_r, win_r = brt.cover_camera(w, h, 1024, 8, brt.Raytracing.Pure, 0.25)
    ref, _ = oracle.render(b, lvl_r, cam_r, win_r, w, h)
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(0))
    g = dr.guides(oracle, b, cam, w, h)
    c = tr.Camera(oracle, cam, w, h)
    sid, ties = tr.sphere_ids(g, c, b.models)
    sph = tr.spheres_of(b.models)
    hist = tr.History()
    for i in range(8):
        lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(i))
        noisy, _ = oracle.render(b, lvl, cam, win, w, h)
        if i == 0:
            single = dr.denoise_frame(oracle, noisy, g, cam)
        out = tr.frame_step(hist, noisy, g, sid, c, sph, 4, True)
    ratio = dr.hit_mse(out, ref, g) / dr.hit_mse(single, ref, g)
    print(f"restatement quality, 8 still frames at 4 spp: {ratio:.3f} of one denoised frame ({ties.sum()} ties)")
    assert ratio <= CPU_BAR, ratio


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _hit(g):
    return g[..., 3] < np.inf


def _device_frame(plugin, lvl, cam, win, w, h, flags, fmt=brt.FLAG_OUT_RGBA32F):
    import torch
    out = torch.zeros((h, w * brt.OUT_PIXEL_BYTES[fmt] // 4), dtype=torch.int32, device="cuda")
    plugin.node.render_device(lvl, cam, win, w, h, out.data_ptr(), flags=flags | fmt)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint8).reshape(h, w, -1)


@pytest.fixture
def fresh(plugin):
    plugin.set_temporal()
    plugin.set_denoise()
    yield plugin
    plugin.set_temporal()


@pytest.mark.gpu
def test_first_frame_equals_the_frame_without_the_flag(fresh):
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 200, 120
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, 0.5)
    p.node.write_buffers(b)
    for fmt in FORMATS:
        want = _device_frame(p, lvl, cam, win, w, h, brt.FLAG_DENOISE, fmt)
        p.reset_temporal()
        got = _device_frame(p, lvl, cam, win, w, h, brt.FLAG_DENOISE | brt.FLAG_TEMPORAL, fmt)
        assert np.array_equal(got, want), fmt
        plain = _device_frame(p, lvl, cam, win, w, h, 0, fmt)
        p.reset_temporal()
        got = _device_frame(p, lvl, cam, win, w, h, brt.FLAG_TEMPORAL, fmt)
        assert np.array_equal(got, plain), fmt
    plain = p.node.run(lvl, cam, win, w, h).copy()
    p.reset_temporal()
    assert np.array_equal(p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_TEMPORAL).view(np.uint32), plain.view(np.uint32))
    st = p.debug_temporal_state(w, h)
    assert (st[..., 3][_hit(p.debug_denoise_guides(cam, win, w, h))] == 1).all() and np.isnan(st[..., 6]).all()


@pytest.mark.gpu
def test_still_frames_accumulate_to_the_mean(fresh):
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 240, 136
    p.node.write_buffers(b)
    p.reset_temporal()
    plains = []
    for i in range(8):
        lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(i))
        plains.append(p.node.run(lvl, cam, win, w, h).copy())
        acc = p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_TEMPORAL).copy()
    g = p.debug_denoise_guides(cam, win, w, h)
    hit = _hit(g) & np.isfinite(np.array(plains)).all(axis=(0, 3))
    mean = np.mean(np.array(plains, np.float64), axis=0)
    err = np.abs(acc[..., :3][hit] - mean[..., :3][hit]) / np.maximum(np.abs(mean[..., :3][hit]), 1e-6)
    assert err.max() <= 1e-5, float(err.max())
    st = p.debug_temporal_state(w, h)
    assert (st[..., 3][hit] == 8).all()
    sky = ~_hit(g)
    assert sky.any() and np.array_equal(acc[sky].view(np.uint32), plains[-1][sky].view(np.uint32))


def _orbit(w, h, spp, i, step_deg, seed_i=None):
    a = np.radians(step_deg * i)
    x, z = 13.0 * np.cos(a) - 3.0 * np.sin(a), 13.0 * np.sin(a) + 3.0 * np.cos(a)
    return uniforms(w, h, spp, 8, (float(x), 2.0, float(z)), (0.0, 0.0, 0.0), 0.4, _seed(i if seed_i is None else seed_i))


def _compare_state(got, want, check):
    """n and the rejections exact, x', y' within 1e-4 px, on the pixels `check`."""
    ng, nw = got[..., 3][check], want[..., 3][check]
    assert np.array_equal(ng, nw), f"n differs at {int((ng != nw).sum())} pixels"
    xg, xw = got[..., 6:8][check], want[..., 6:8][check]
    assert np.array_equal(np.isnan(xg), np.isnan(xw))
    ok = ~np.isnan(xw)
    assert np.abs(xg[ok] - xw[ok]).max(initial=0) <= 1e-4


def _rel(got, want):
    return float((np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())


@pytest.mark.gpu
@pytest.mark.parametrize("denoise_on", [False, True])
def test_orbit_matches_the_restatement(fresh, oracle, denoise_on):
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 320, 180
    p.node.write_buffers(b)
    p.reset_temporal()
    hist = tr.History()
    sph = tr.spheres_of(b.models)
    flags = brt.FLAG_TEMPORAL | (brt.FLAG_DENOISE if denoise_on else 0)
    n_ties = 0
    for i in range(5):
        lvl, cam, win = _orbit(w, h, 4, i, 0.25)
        plain = p.node.run(lvl, cam, win, w, h).copy()
        got = p.node.run(lvl, cam, win, w, h, flags=flags).copy()
        g = p.debug_denoise_guides(cam, win, w, h)
        c = tr.Camera(oracle, cam, w, h)
        sid, ties = tr.sphere_ids(g, c, b.models)
        n_ties += int(ties.sum())
        want = tr.frame_step(hist, plain, g, sid, c, sph, 4, denoise_on)
        _compare_state(p.debug_temporal_state(w, h), tr.state(hist), ~ties)
        assert _rel(got, want) <= 1e-4
        if i > 0:
            kept = tr.state(hist)[..., 3] >= 2
            assert kept.sum() > 0.5 * _hit(g).sum()                   # (the orbit keeps most of the history)
    print(f"orbit: {n_ties} brute-force ties")
    assert n_ties <= 0.001 * w * h * 5


def _moved(b, k, delta):
    models = b.models.copy()
    models[k]["position"] = models[k]["position"] + np.asarray(delta, F32)
    return brt.Buffers(models, b.materials, None)


@pytest.mark.gpu
def test_a_moving_sphere_keeps_its_history(fresh, oracle):
    """One of the three big spheres moves between uploads: the restatement agrees, >= 90 % of its pixels that stay visible keep their
    history, and without the motion term fewer than half would."""
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 320, 180
    big = int(np.argsort(-b.models["radius"], kind="stable")[1])    # (a big sphere: the largest after the ground)
    sph0 = tr.spheres_of(b.models)
    b1 = _moved(b, big, (0.5, 0.0, 0.3))                            # towards the camera and ~10 px sideways
    sph1 = tr.spheres_of(b1.models)
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(0))
    c = tr.Camera(oracle, cam, w, h)
    p.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    p.reset_temporal()
    f0 = p.node.run(lvl, cam, win, w, h).copy()
    p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_TEMPORAL)
    g0 = p.debug_denoise_guides(cam, win, w, h)
    sid0, t0 = tr.sphere_ids(g0, c, b.models)
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(1))
    p.node.write_buffers(b1)
    f1 = p.node.run(lvl, cam, win, w, h).copy()
    got = p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_TEMPORAL).copy()
    g1 = p.debug_denoise_guides(cam, win, w, h)
    sid1, t1 = tr.sphere_ids(g1, c, b1.models)
    results = {}
    for motion in (True, False):
        hist = tr.History()
        tr.frame_step(hist, f0, g0, sid0, c, sph0, 4, False)
        want = tr.frame_step(hist, f1, g1, sid1, c, sph1, 4, False, motion=motion)
        results[motion] = (tr.state(hist), want)
    st = p.debug_temporal_state(w, h)
    _compare_state(st, results[True][0], ~(t0 | t1))
    assert _rel(got, results[True][1]) <= 1e-4
    # its pixels whose surface point was visible before too: X - delta projected into the (same) camera lands on the sphere at the
    # distance of that point (nearest pixel, 5 %)
    mine = (sid1 == big) & ~t1
    x = (c.o + g1[..., 3][..., None] * c.dirs)[mine] - np.asarray((0.5, 0.0, 0.3), F32)
    v = (x - c.o).astype(F32)
    inv = c.inverse()
    z, sx, sy = (v @ inv[k] for k in range(3))
    qx = np.rint((((sx / z) / c.tan / c.aspect + 1) * 0.5) * w - 0.5).astype(np.int64)
    qy = np.rint(((1 - (sy / z) / c.tan) * 0.5) * h - 0.5).astype(np.int64)
    inside = (z > 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
    dist = np.sqrt((v * v).sum(-1))
    seen = inside & (sid0[qy, qx] == big) & (np.abs(g0[qy, qx, 3] - dist) <= 0.05 * dist)
    both = np.zeros((h, w), bool)
    both[mine] = seen
    assert both.sum() > 500
    keep = (st[..., 3][both] == 2).mean()
    keep_static = (results[False][0][..., 3][both] == 2).mean()
    print(f"moving sphere: {keep:.3f} keep their history with the motion term, {keep_static:.3f} without")
    assert keep >= 0.9 and keep_static < 0.5
    p.node.write_buffers(b)


@pytest.mark.gpu
def test_lifecycle(fresh):
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 160, 96
    lvl, cam, win = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(0))
    lvl2, cam2, win2 = brt.cover_camera(w, h, 4, 8, brt.Raytracing.Pure, _seed(1))
    p.node.write_buffers(b)
    first = p.node.run(lvl2, cam2, win2, w, h, flags=brt.FLAG_DENOISE).copy()         # (a): what a frame with no history gives

    def accumulate_then(reset):
        p.reset_temporal()
        p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE | brt.FLAG_TEMPORAL)
        reset()
        return p.node.run(lvl2, cam2, win2, w, h, flags=brt.FLAG_DENOISE | brt.FLAG_TEMPORAL).copy()

    assert not np.array_equal(accumulate_then(lambda: None), first)
    assert np.array_equal(accumulate_then(p.reset_temporal).view(np.uint32), first.view(np.uint32))
    assert np.array_equal(accumulate_then(lambda: p.set_temporal(16)).view(np.uint32), first.view(np.uint32))
    # resize: a frame of another size in between
    lvl_s, cam_s, win_s = brt.cover_camera(w // 2, h // 2, 4, 8, brt.Raytracing.Pure, _seed(2))
    got = accumulate_then(lambda: p.node.run(lvl_s, cam_s, win_s, w // 2, h // 2, flags=brt.FLAG_TEMPORAL))
    assert np.array_equal(got.view(np.uint32), first.view(np.uint32))
    # an upload with another sphere count (and back)
    fewer = brt.Buffers(b.models[:-1], b.materials, None)
    got = accumulate_then(lambda: (p.node.write_buffers(fewer), p.node.write_buffers(b)))
    assert np.array_equal(got.view(np.uint32), first.view(np.uint32))
    # a re-upload of the same scene keeps the history
    assert not np.array_equal(accumulate_then(lambda: p.node.write_buffers(b)), first)
    # a plain FLAG_DENOISE frame between temporal frames is the same as in a fresh context, and changes nothing of the sequence
    p.reset_temporal()
    p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE | brt.FLAG_TEMPORAL)
    seq = p.node.run(lvl2, cam2, win2, w, h, flags=brt.FLAG_DENOISE | brt.FLAG_TEMPORAL).copy()
    p.reset_temporal()
    p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE | brt.FLAG_TEMPORAL)
    between = p.node.run(lvl_s, cam_s, win_s, w // 2, h // 2, flags=brt.FLAG_DENOISE).copy()
    between2 = p.node.run(lvl2, cam2, win2, w, h, flags=brt.FLAG_DENOISE).copy()
    assert np.array_equal(between2.view(np.uint32), first.view(np.uint32))
    again = p.node.run(lvl2, cam2, win2, w, h, flags=brt.FLAG_DENOISE | brt.FLAG_TEMPORAL).copy()
    assert np.array_equal(again.view(np.uint32), seq.view(np.uint32))
    with brt.RaytracePlugin([0]) as other:
        other.node.write_buffers(b)
        want = other.node.run(lvl_s, cam_s, win_s, w // 2, h // 2, flags=brt.FLAG_DENOISE)
        assert np.array_equal(between.view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_entry_points_agree(fresh):
    import torch
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 160, 96
    p.node.write_buffers(b)
    for flags in (brt.FLAG_TEMPORAL, brt.FLAG_TEMPORAL | brt.FLAG_DENOISE):
        runs = {}
        for entry in ("run", "device", "denoise_device", "ctx00"):
            seq = []
            q = p
            if entry == "ctx00":
                q = brt.RaytracePlugin([0, 0])
                q.node.write_buffers(b)
            q.reset_temporal()
            for i in range(3):
                lvl, cam, win = _orbit(w, h, 4, i, 0.5)
                if entry in ("run", "ctx00"):
                    seq.append(q.node.run(lvl, cam, win, w, h, flags=flags).copy())
                    continue
                frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
                if entry == "device":
                    q.node.render_device(lvl, cam, win, w, h, frame.data_ptr(), flags=flags)
                else:
                    q.node.render_device(lvl, cam, win, w, h, frame.data_ptr())
                    q.node.denoise_device(cam, win, w, h, frame.data_ptr(), frame.data_ptr(), flags=flags)
                torch.cuda.synchronize()
                seq.append(frame.cpu().numpy())
            if entry == "ctx00":
                q.close()
            runs[entry] = np.array(seq)
        for entry, seq in runs.items():
            assert np.array_equal(seq.view(np.uint32), runs["run"].view(np.uint32)), (flags, entry)


@pytest.mark.gpu
def test_rejections(fresh):
    import torch
    p = fresh
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 64, 40
    p.node.write_buffers(b)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    for level in (brt.Raytracing.Skip, brt.Raytracing.FallbackRaster, brt.Raytracing.FallbackRaytraced):
        lvl, cam, win = brt.cover_camera(w, h, 2, 4, level)
        for flags in (brt.FLAG_TEMPORAL, brt.FLAG_TEMPORAL | brt.FLAG_DENOISE):
            with pytest.raises(brt.BrtError) as e:
                p.node.run(lvl, cam, win, w, h, flags=flags)
            assert e.value.code == ERR_UNSUPPORTED
            with pytest.raises(brt.BrtError) as e:
                p.node.render_device(lvl, cam, win, w, h, frame.data_ptr(), flags=flags)
            assert e.value.code == ERR_UNSUPPORTED
    lvl, cam, win = brt.cover_camera(w, h, 2, 4)
    with pytest.raises(brt.BrtError) as e:
        p.node.render_part_device(lvl, cam, win, w, h, 0, 1, frame.data_ptr(), flags=brt.FLAG_TEMPORAL)
    assert e.value.code == ERR_UNSUPPORTED
    with pytest.raises(brt.BrtError) as e:
        p.node.deinterleave_device(frame.data_ptr(), 1, w, h, frame.data_ptr(), out_format=brt.FLAG_TEMPORAL)
    assert e.value.code == ERR_UNSUPPORTED
    for m in (0, 65536, 1 << 31):
        with pytest.raises(brt.BrtError) as e:
            p.set_temporal(m)
        assert e.value.code == ERR_INVALID
    p.set_temporal(65535)
    p.set_temporal(1)
    with pytest.raises(brt.BrtError) as e:                              # a history of another size
        p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_TEMPORAL)
        p.debug_temporal_state(w + 1, h)
    assert e.value.code == ERR_INVALID


def _quality(p, b, w, h, spp, orbit_step):
    _, cam_r, win_r = brt.cover_camera(w, h, 1024, 8, brt.Raytracing.Pure, 0.25)
    p.node.write_buffers(b)
    p.reset_temporal()
    for i in range(8):
        if orbit_step:
            lvl, cam, win = _orbit(w, h, spp, i, orbit_step)
        else:
            lvl, cam, win = brt.cover_camera(w, h, spp, 8, brt.Raytracing.Pure, _seed(i))
        out = p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_TEMPORAL | brt.FLAG_DENOISE).copy()
    single = p.node.run(lvl, cam, win, w, h, flags=brt.FLAG_DENOISE).copy()
    noisy = p.node.run(lvl, cam, win, w, h).copy()
    if orbit_step:
        lvl_r, cam_r, win_r = _orbit(w, h, 1024, 7, orbit_step, seed_i=-7)
    ref = p.node.run(lvl, cam_r, win_r, w, h).copy()
    g = p.debug_denoise_guides(cam, win, w, h)
    return dr.hit_mse(out, ref, g) / dr.hit_mse(single, ref, g), dr.hit_mse(out, ref, g) / dr.hit_mse(noisy, ref, g)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["still4", "still64", "orbit4"])
def test_quality_on_the_gpu(fresh, case):
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    spp = 64 if case == "still64" else 4
    ratio, vs_noisy = _quality(fresh, b, 480, 270, spp, 0.25 if case == "orbit4" else 0.0)
    print(f"quality {case}: {ratio:.3f} of one denoised frame, {vs_noisy:.3f} of the noisy frame")
    assert ratio <= GPU_BARS[case], ratio
