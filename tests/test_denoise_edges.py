"""The denoiser on the GPU (brt_denoise_device, BRT_FLAG_DENOISE) against the float64 reference (tests/denoise_ref64.py) at the shapes,
sample counts and inputs where a tiled filter goes wrong: partial 16-pixel tiles, frames smaller than the 7x7 window or the a-trous
footprint, both sides of the strength switch, NaN / Inf / overflowing / negative / huge colours and alpha != 1; pass-through bits, the
all-NaN frame of sample_count = 0, the store formats at an odd shape, and the guides under the hot order of a scene larger than the LDS."""
import numpy as np
import pytest

import bevyray_amd as brt
import denoise_ref as dr
import denoise_ref64 as d64

F32 = np.float32
BAR = 1e-4
SHAPES = [(1, 1), (1, 40), (40, 1), (7, 5), (15, 16), (16, 15), (17, 17), (31, 33), (65, 7), (200, 117), (641, 361), (4096, 3)]
ALL_ITERATIONS = {(17, 17), (200, 117)}


def _frame(plugin, w, h, spp, bounces=4, seed=0.5):
    lvl, cam, win = brt.cover_camera(w, h, spp, bounces, brt.Raytracing.Pure, seed)
    return lvl, cam, win, plugin.node.run(lvl, cam, win, w, h).copy()


def _denoise_dev(plugin, cam, win, w, h, frame, out_format=brt.FLAG_OUT_RGBA32F):
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    out = torch.zeros((h, w * brt.OUT_PIXEL_BYTES[out_format] // 4), dtype=torch.int32, device="cuda")
    plugin.node.denoise_device(cam, win, w, h, d_in.data_ptr(), out.data_ptr(), out_format=out_format)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint8).reshape(h, w, -1)


def _check(got, want, frame, g, what):
    """live pixels within BAR of the reference, pass-through pixels the input's bits."""
    through = d64.passes_through(frame, g)
    err = d64.rel_err(got, want, ~through)
    bad = np.argwhere((d64.rel_err(got, want) > BAR) & ~through)
    assert err.size == 0 or err.max() <= BAR, (what, float(err.max()), bad[:4].tolist())
    assert np.array_equal(got[through].view(np.uint32), frame[through].view(np.uint32)), what


@pytest.fixture
def cover(plugin):
    plugin.node.write_buffers(brt.generate_scene(brt.SCENE_COVER, 1))
    plugin.set_denoise()
    yield plugin
    plugin.set_denoise()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_filter_shapes(cover, oracle, w, h):
    p = cover
    _, cam, win, frame = _frame(p, w, h, 4)
    g = p.debug_denoise_guides(cam, win, w, h)
    if w * h <= 1200:                                        # (the guides at partial tiles: the oracle's raycast, bitwise)
        want_g = dr.guides(oracle, brt.generate_scene(brt.SCENE_COVER, 1), cam, w, h)
        assert np.array_equal(g.view(np.uint32), want_g.view(np.uint32))
    _, dirs, tan = dr.pixel_center_rays(oracle, cam, w, h)
    for it in (range(1, 7) if (w, h) in ALL_ITERATIONS else (1, 6)):
        p.set_denoise(it)
        got = _denoise_dev(p, cam, win, w, h, frame).view(F32)
        want = d64.denoise(frame, g, dirs, tan, spp=4, **{**dr.DEFAULTS, "iterations": it})
        _check(got, want, frame, g, (w, h, it))


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4, 5, 16, 1024])
def test_filter_sample_counts(cover, oracle, spp):
    """both sides of kStrengthSpp = 4: the strength and sigma_l scale by sqrt(4 / spp) from 5 spp on."""
    p = cover
    w, h = 97, 61
    _, cam, win, frame = _frame(p, w, h, spp)
    g = p.debug_denoise_guides(cam, win, w, h)
    _, dirs, tan = dr.pixel_center_rays(oracle, cam, w, h)
    for it in (1, 5):
        p.set_denoise(it)
        got = _denoise_dev(p, cam, win, w, h, frame).view(F32)
        _check(got, d64.denoise(frame, g, dirs, tan, spp=spp, **{**dr.DEFAULTS, "iterations": it}), frame, g, (spp, it))
        assert np.abs(got - frame)[~d64.passes_through(frame, g)].max() > 1e-4          # (it did filter)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(200, 117), (31, 33)])
def test_injected_values(cover, oracle, w, h):
    """NaN and +-Inf pixels, a finite colour whose c / a overflows, negative colours, fireflies up to 1e6 and alpha != 1: within the bar
    of the reference; the non-finite and overflowing pixels come out as their input's bits, and no neighbour turns non-finite.

    A handful of pixels right next to a firefly of 1e2 .. 1e6 need more than the bar against float64 from the second pass on (measured
    at 3 passes: up to 3.4e-3 at 31x33 and 2.7e-4 at 200x117): the result there is dominated by a tiny weight times a colour 1e2 .. 1e6
    times larger, so the f32 rounding inside that weight shows up ~1e3 times larger in the result.  It is the f32 arithmetic the filter
    is specified in, not the kernel: at exactly those pixels the f32 restatement (denoise_ref.py) lands where the GPU does, within the bar.
    So a pixel over the bar must lie within the reach of the passes from such a firefly, match the f32 restatement, and be one of at
    most 8; every other pixel holds the bar."""
    p = cover
    _, cam, win, frame = _frame(p, w, h, 4)
    g = p.debug_denoise_guides(cam, win, w, h)
    f = d64.inject(frame, g, seed=w)
    through = d64.passes_through(f, g)
    hit = g[..., 3] < np.inf
    assert (through & hit).sum() >= 3 and (f[..., 3] != 1).any() and (f[..., :3] < 0).any()
    _, dirs, tan = dr.pixel_center_rays(oracle, cam, w, h)
    big = (np.abs(np.nan_to_num(f[..., :3], posinf=0, neginf=0)) >= 100).any(-1) & ~through
    for it in (1, 3, 6):
        reach = 2 * ((1 << it) - 1)                          # (how far a value travels through `it` passes)
        near = np.zeros_like(big)
        for y, x in np.argwhere(big):
            near[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = True
        p.set_denoise(it)
        got = _denoise_dev(p, cam, win, w, h, f).view(F32)
        settings = {**dr.DEFAULTS, "iterations": it}
        want = d64.denoise(f, g, dirs, tan, spp=4, **settings)
        over = (d64.rel_err(got, want) > BAR) & ~through
        assert not (over & ~near).any(), (it, np.argwhere(over & ~near)[:4].tolist())
        if over.any():
            want32 = dr.denoise(f, g, dirs, tan, spp=4, **settings)
            assert d64.rel_err(got, want32, over).max() <= BAR, it
            assert over.sum() <= 8, (it, int(over.sum()))
        _check(got, np.where(over[..., None], got, want), f, g, it)
        assert np.isfinite(got[~through]).all()
        assert np.array_equal(got[..., 3].view(np.uint32), f[..., 3].view(np.uint32))          # (alpha is carried through aux.x)


@pytest.mark.gpu
def test_beyond_the_finite_range(cover, oracle):
    """Fireflies of 1e20 and 1e30, where l^2 overflows f32 in the variance (and w^2 var overflows in the passes): the kernel's rule is
    max_f(0, NaN) = 0 (fmaxf), so a NaN or infinite variance only switches the luminance term off around it -- every hit pixel with a
    finite input comes out finite, and the pass-through pixels keep their bits."""
    p = cover
    w, h = 64, 48
    _, cam, win, frame = _frame(p, w, h, 4)
    g = p.debug_denoise_guides(cam, win, w, h)
    hit = np.argwhere(g[..., 3] < np.inf)
    f = frame.copy()
    for i, (y, x) in enumerate(hit[:: max(1, len(hit) // 12)][:12]):
        f[y, x, :3] = F32(1e20 if i % 2 else 1e30)
    f[hit[5][0], hit[5][1], 0] = np.nan
    through = d64.passes_through(f, g)
    for it in range(1, 7):
        p.set_denoise(it)
        got = _denoise_dev(p, cam, win, w, h, f).view(F32)
        assert np.isfinite(got[~through]).all(), (it, np.argwhere(~np.isfinite(got).all(-1) & ~through)[:4].tolist())
        assert np.array_equal(got[through].view(np.uint32), f[through].view(np.uint32))
    # one pass: more than 6 px from the fireflies (the 7x7 variance, then the 3x3 Gaussian and the 5x5 taps) the reference still holds
    p.set_denoise(1)
    got = _denoise_dev(p, cam, win, w, h, f).view(F32)
    _, dirs, tan = dr.pixel_center_rays(oracle, cam, w, h)
    want = d64.denoise(f, g, dirs, tan, spp=4, **{**dr.DEFAULTS, "iterations": 1})
    huge = (np.abs(np.nan_to_num(f[..., :3])) > 1e10).any(-1)
    near = np.zeros_like(huge)
    for y, x in np.argwhere(huge):
        near[max(0, y - 6):y + 7, max(0, x - 6):x + 7] = True
    assert d64.rel_err(got, want, ~near & ~through).max() <= BAR


@pytest.mark.gpu
def test_sample_count_zero_frame_passes_every_flag(cover):
    """sample_count = 0 renders 0 / 0 = NaN everywhere: every pixel passes through, so DENOISE, TEMPORAL and both give the bits of the
    frame without a flag (and a temporal frame of it leaves no history)."""
    from helpers import uniforms
    p = cover
    w, h = 37, 21
    lvl, cam, win = uniforms(w, h, 0, 4, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 0.4, 0.5)
    plain = p.node.run(lvl, cam, win, w, h).copy()
    assert np.isnan(plain[..., :3]).all()
    for flags in (brt.FLAG_DENOISE, brt.FLAG_TEMPORAL, brt.FLAG_DENOISE | brt.FLAG_TEMPORAL):
        p.reset_temporal()
        for _ in range(2):
            got = p.node.run(lvl, cam, win, w, h, flags=flags)
            assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), flags
        if flags & brt.FLAG_TEMPORAL:
            assert (p.debug_temporal_state(w, h)[..., 3] == 0).all()
    p.reset_temporal()


@pytest.mark.gpu
def test_output_formats_at_an_odd_shape(cover, oracle):
    p = cover
    w, h = 33, 19
    _, cam, win, frame = _frame(p, w, h, 4)
    g = p.debug_denoise_guides(cam, win, w, h)
    f = d64.inject(frame, g, seed=7)
    for it in (1, 6):
        p.set_denoise(it)
        f32 = _denoise_dev(p, cam, win, w, h, f).view(F32)
        for fmt, name in ((brt.FLAG_OUT_RGBA8_UNORM_SRGB, "srgb8"), (brt.FLAG_OUT_RGBA8_UNORM, "unorm8"), (brt.FLAG_OUT_RGBA16F, "f16")):
            got = _denoise_dev(p, cam, win, w, h, f, out_format=fmt)
            want = oracle.encode_frame(f32, name)
            assert np.array_equal(got.view(want.dtype).reshape(want.shape), want), (it, name)


@pytest.mark.gpu
def test_guides_under_the_hot_order(oracle):
    """The stress grid (10 004 spheres, top of the tree in the LDS) at 64 spp: once the records are numbered by visits (hot_records >
    1000) the resident spheres are renumbered; the guides -- material ids included -- still equal the oracle's raycast on the CPU twin
    of the tree, and again after a camera move that has them counted again."""
    from helpers import uniforms
    b = brt.generate_scene(brt.SCENE_STRESS_GRID, 1)
    w, h = 160, 90
    views = [brt.cover_camera(w, h, 64, 4), uniforms(w, h, 64, 4, (-9.0, 4.0, 12.0), (3.0, 0.0, -2.0), 0.6, 0.31)]
    with brt.RaytracePlugin([0]) as p:
        p.node.write_buffers(brt.Buffers(b.models, b.materials, None))
        for i, (lvl, cam, win) in enumerate(views):
            for _ in range(3):
                p.node.run(lvl, cam, win, w, h)
            st = dict(p.node.last_stats)
            assert st["scene_in_lds"] == 2 and st["hot_records"] > 1000, (i, st)
            tree = brt.build_bvh_sah(b.models, st["tree_reach"])
            got = p.debug_denoise_guides(cam, win, w, h)
            want = dr.guides(oracle, brt.Buffers(b.models, b.materials, tree), cam, w, h)
            bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
            assert not bad.any(), (i, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert (got[..., 3] < np.inf).sum() > w * h // 4
