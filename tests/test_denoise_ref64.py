"""The numpy f32 restatement of the denoiser (tests/denoise_ref.py, the kernel's order of operations) against the independent float64
reference (tests/denoise_ref64.py, the formulas of DESIGN.md section 10): synthetic guide planes and small oracle frames, every
iteration count, sample counts on both sides of the strength switch.  Bar: |f32 - f64| <= 1e-4 max(1, |f64|) per pixel."""
import numpy as np
import pytest

import bevyray_amd as brt
import denoise_ref as dr
import denoise_ref64 as d64

F32 = np.float32
BAR = 1e-4
SPPS = (1, 4, 5, 1024)


def _planes(h, w, rng):
    """The synthetic cases: (name, frame, guides, dirs) over a flat camera looking down -z."""
    dirs = np.zeros((h, w, 3), F32)
    dirs[..., 2] = -1
    base = np.zeros((h, w, 8), F32)
    base[..., 2] = 1.0
    base[..., 3] = 5.0
    base[..., 4:7] = (0.5, 0.6, 0.7)
    noisy = np.ones((h, w, 4), F32)
    noisy[..., :3] = 0.4 + 0.15 * rng.standard_normal((h, w, 3)).astype(F32)
    cases = []
    g = base.copy()
    g[:, w // 2:, 0:3] = (0.8, 0.0, 0.6)                                   # a normal step of ~53 degrees
    cases.append(("normal_step", noisy, g))
    g = base.copy()
    g[h // 2:, :, 3] = 5.5                                                 # a depth step
    g[:, : w // 3, 3] += np.linspace(0, 0.3, w // 3, dtype=F32)[None, :]   # and a slope
    cases.append(("depth_step", noisy, g))
    g = base.copy()
    holes = rng.random((h, w)) < 0.15
    holes[: h // 4, : w // 4] = True
    g[holes, 0:4] = (0, 0, 0, np.inf)
    g[holes, 4:7] = 1
    g[holes, 7:8] = np.array([0xFFFFFFFF], np.uint32).view(F32)
    sky = noisy.copy()
    sky[holes, :3] = (0.7, 0.8, 1.0)
    cases.append(("sky_holes", sky, g))
    const = np.ones((h, w, 4), F32)
    const[..., :3] = (0.3, 0.45, 0.6)
    cases.append(("constant", const, base))
    g = base.copy()
    n = rng.standard_normal((h, w, 3)).astype(F32) * F32(0.15) + np.array([0, 0, 1], F32)
    g[..., 0:3] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    g[..., 3] = 5.0 + 0.05 * rng.standard_normal((h, w)).astype(F32)
    field = np.ones((h, w, 4), F32)
    field[..., :3] = np.abs(rng.standard_normal((h, w, 3))).astype(F32) * F32(2.0)
    cases.append(("noise_field", field, g))
    return [(name, f, g, dirs) for name, f, g in cases]


def _check(got32, want64, through, what):
    err = d64.rel_err(got32, want64, ~through)
    assert err.size == 0 or err.max() <= BAR, (what, float(err.max()), np.argwhere(d64.rel_err(got32, want64) > BAR)[:4].tolist())
    assert np.array_equal(got32[through].view(np.uint32), np.asarray(want64[through], F32).view(np.uint32)), what


def test_synthetic_planes_every_iteration_count():
    rng = np.random.default_rng(11)
    for name, frame, g, dirs in _planes(23, 37, rng):                      # (a partial tile both ways)
        through = d64.passes_through(frame, g)
        for it in range(1, 7):
            for spp in SPPS:
                got = dr.denoise(frame, g, dirs, 0.2, iterations=it, spp=spp)
                want = d64.denoise(frame, g, dirs, 0.2, iterations=it, spp=spp)
                _check(got, want, through, (name, it, spp))


def test_constant_image_stays_constant_in_float64():
    rng = np.random.default_rng(12)
    (_, frame, g, dirs), = [c for c in _planes(16, 16, rng) if c[0] == "constant"]
    for it in (1, 6):
        out = d64.denoise(frame, g, dirs, 0.2, iterations=it, spp=5)
        assert np.abs(out - frame).max() <= 1e-12


def test_strength_switch_sits_at_four_samples():
    assert d64.strength(1) == d64.strength(4) == 1.0 and d64.strength(5) == pytest.approx(np.sqrt(0.8)) and d64.strength(1024) == 1 / 16
    for spp in (1, 4, 5, 16, 1024):
        assert float(dr.strength(spp)) == pytest.approx(d64.strength(spp), rel=1e-7)


def test_nan_rules_follow_fmax():
    """max(0, NaN) is 0 where the kernel calls max_f: a tap whose variance is NaN (w = 0 times an infinite variance) does not turn the
    pixel's luminance scale into NaN; the restatement follows the same rule."""
    h, w = 12, 12
    dirs = np.zeros((h, w, 3), F32)
    dirs[..., 2] = -1
    g = np.zeros((h, w, 8), F32)
    g[..., 2], g[..., 3], g[..., 4:7] = 1.0, 5.0, 1.0
    g[:, 6:, 0:3] = (1.0, 0.0, 0.0)                                        # w_n = 0 across the step
    frame = np.ones((h, w, 4), F32)
    frame[..., :3] = 0.5
    frame[3, 3, :3] = 1e20                                                # l^2 overflows in f32
    for it in (1, 3, 6):
        out = dr.denoise(frame, g, dirs, 0.2, iterations=it)
        assert np.isfinite(out).all(), it
        assert np.isfinite(d64.denoise(frame, g, dirs, 0.2, iterations=it)).all()


@pytest.fixture(scope="module")
def cover_small(oracle):
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 64, 36
    out = {}
    for spp in (4, 64):
        lvl, cam, win = brt.cover_camera(w, h, spp, 8, brt.Raytracing.Pure, 0.5)
        frame, _ = oracle.render(b, lvl, cam, win, w, h)
        out[spp] = (frame, cam)
    g = dr.guides(oracle, b, out[4][1], w, h)
    _, dirs, tan = dr.pixel_center_rays(oracle, out[4][1], w, h)
    return out, g, dirs, tan


@pytest.mark.parametrize("rendered_spp", [4, 64])
def test_oracle_frames_every_iteration_count(cover_small, rendered_spp):
    frames, g, dirs, tan = cover_small
    frame = frames[rendered_spp][0]
    through = d64.passes_through(frame, g)
    assert (~through).sum() > frame.shape[0] * frame.shape[1] // 2
    for it in range(1, 7):
        for spp in SPPS:
            got = dr.denoise(frame, g, dirs, tan, iterations=it, spp=spp)
            want = d64.denoise(frame, g, dirs, tan, iterations=it, spp=spp)
            _check(got, want, through, (rendered_spp, it, spp))
    # a non-default set of sigmas
    got = dr.denoise(frame, g, dirs, tan, iterations=4, sigma_l=2.5, sigma_n=32.0, sigma_z=0.5, spp=rendered_spp)
    want = d64.denoise(frame, g, dirs, tan, iterations=4, sigma_l=2.5, sigma_n=32.0, sigma_z=0.5, spp=rendered_spp)
    _check(got, want, through, "sigmas")


def test_oracle_frame_with_injected_values(cover_small):
    """NaN / +-Inf, a finite colour whose c / a overflows, negative colours, fireflies up to 1e6 and alpha != 1."""
    frames, g, dirs, tan = cover_small
    frame = d64.inject(frames[4][0], g)
    assert (d64.passes_through(frame, g) & np.isfinite(frame[..., :3]).all(-1) & (g[..., 3] < np.inf)).any()   # (a c / a overflow)
    through = d64.passes_through(frame, g)
    for it in (1, 6):
        got = dr.denoise(frame, g, dirs, tan, iterations=it, spp=4)
        want = d64.denoise(frame, g, dirs, tan, iterations=it, spp=4)
        _check(got, want, through, it)
