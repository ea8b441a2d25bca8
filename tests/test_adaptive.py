"""Adaptive sampling (brt_set_adaptive, brt_render_adaptive_device, brt_adaptive_refine_device, brt_adaptive_mask_device,
brt_host_adaptive_class; DESIGN.md "Adaptive sampling").  CPU: the exports and brt_set_adaptive's rejections, the host rule against the
restatement (tests/adaptive_ref.py) on random tap sets, properties of the restatement on oracle frames, the quality bar.  GPU: the mask
against the restatement on every pixel, the frame bitwise against two oracle frames and the GPU's own mask, edge cases, the one-call
form against its steps, a scene of 32-bit descriptors, unchanged paths and the dispatch-order history, caller streams, refusals."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import adaptive_ref as ar
import bevyray_amd as brt
import denoise_ref as dr
from bevyray_amd import _lib
from helpers import big_scene, big_view, make_buffers, resident_callee_tree, uniforms

F32 = np.float32
ERR_INVALID, ERR_NO_SCENE, ERR_UNSUPPORTED = -1, -7, -8
DEFAULTS = (8, brt.ADAPT_DEFAULT_THRESHOLD, 6)
FORMATS = {brt.FLAG_OUT_RGBA32F: None, brt.FLAG_OUT_RGBA8_UNORM_SRGB: "srgb8", brt.FLAG_OUT_RGBA16F: "f16", brt.FLAG_OUT_RGBA8_UNORM: "unorm8"}
# Quality (test_restatement_quality_bar): R = MSE of the adaptive frame / MSE of the uniform frame at ceil(8 + 64 s) spp, both against
# 1024 spp of another window seed; cover scene, 96x54, 8 bounces, base 8, full 64, min_taps 6, on the oracle.  Measured on the grid
# 0.0125 .. 1.6 (doubling): 0.9299, 0.8862, 0.8905, 1.0403, 1.6795, 1.9420, 1.4688, 1.3489.  The default threshold is the grid point of
# the lowest R, 0.025; R < 1 only where three quarters of the frame are selected (DESIGN.md section 17 says what that means).
GRID = (0.0125, 0.025, 0.05, 0.1, 0.2, 0.4, 0.8, 1.6)
R_DEFAULT = 0.8862
BAR = min(1.1 * R_DEFAULT, 0.999)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_exports_and_set_adaptive_rejections():
    lib = _lib.load()
    for name in ("brt_set_adaptive", "brt_render_adaptive_device", "brt_adaptive_refine_device", "brt_adaptive_mask_device",
                 "brt_host_adaptive_class"):
        assert hasattr(lib, name), name
    assert lib.brt_abi_version() == 6
    assert (brt.ADAPT_SPARSE, brt.ADAPT_NOISY) == (ar.SPARSE, ar.NOISY) == (1, 2)
    assert lib.brt_set_adaptive(None, 8, 0.5, 6) == ERR_INVALID
    c = C.c_uint32(0)
    assert lib.brt_host_adaptive_class(1.0, 0, None, None, None, None, 0.5, 6, C.byref(c)) == ERR_INVALID


def _random_case(rng, kind):
    """One pixel and its 25 taps.  -> (t, id, rgb, inside (25,), ids (25,), cols (25, 3))"""
    ids = np.where(rng.random(25) < 0.7, 5, rng.integers(0, 4, 25)).astype(np.uint32)
    inside = rng.random(25) < 0.85
    cols = (rng.random((25, 3)) * rng.choice([0.004, 0.05, 1.0, 40.0])).astype(F32)
    if kind == "constant":
        cols[:] = cols[12]
    elif kind == "nonfinite":
        bad = rng.random(25) < 0.3
        cols[bad, rng.integers(0, 3)] = rng.choice([np.inf, -np.inf, np.nan])
    elif kind == "dark":
        cols *= F32(0.001)
    ids[12], inside[12] = 5, True
    t = F32(np.inf) if kind == "sky" else F32(3.0)
    return t, 5, cols[12].copy(), inside, ids, cols


def test_host_rule_equals_the_restatement_on_random_taps():
    rng = np.random.default_rng(17)
    seen = set()
    for i in range(1500):
        kind = ("plain", "constant", "nonfinite", "dark", "sky", "own_nonfinite")[i % 6]
        t, pid, rgb, inside, ids, cols = _random_case(rng, "plain" if kind == "own_nonfinite" else kind)
        if kind == "own_nonfinite":
            cols[12, 1] = rgb[1] = F32(np.nan)
        thr, mt = float(rng.choice([0.02, 0.1, 0.5, 2.0])), int(rng.integers(1, 26))
        ls = ar.luma(cols)
        want = ar.class_from_taps(t, pid, ar.luma(rgb), inside, ids, ls, thr, mt)
        assert brt.adaptive_class(t, pid, rgb, inside, ids, cols, thr, mt) == want, (i, kind)
        # n = min_taps - 1 / min_taps: the boundary of SPARSE
        n = int((inside & (ids == pid) & np.isfinite(ls)).sum())
        if kind in ("plain", "constant", "dark") and 1 <= n <= 24:
            assert brt.adaptive_class(t, pid, rgb, inside, ids, cols, thr, n + 1) == ar.SPARSE
            got = brt.adaptive_class(t, pid, rgb, inside, ids, cols, thr, n)
            assert got == ar.class_from_taps(t, pid, ar.luma(rgb), inside, ids, ls, thr, n) != ar.SPARSE
        if kind == "constant":
            assert brt.adaptive_class(t, pid, rgb, inside, ids, cols, thr, 1) == 0          # v = 0 is never above thr^2 > 0
        if kind in ("sky", "own_nonfinite"):
            assert want == 0
        seen.add((kind, want))
    assert {("plain", 0), ("plain", 1), ("plain", 2), ("dark", 2), ("nonfinite", 1)} <= seen, seen


def test_host_rule_mean_floor():
    """m below 0.01: thr = threshold * 0.01, not threshold * m."""
    inside, ids = np.ones(25, bool), np.zeros(25, np.uint32)
    cols = np.zeros((25, 3), F32)
    cols[::2, 1] = F32(0.004)       # luminances 0 and 0.00286: m = 0.0015, std = 0.0014
    for thr, want in ((0.2, 0), (0.1, ar.NOISY)):      # 0.2 * 0.01 = 0.002 > std; with thr * m (0.0003) both would be NOISY
        assert brt.adaptive_class(1.0, 0, cols[0], inside, ids, cols, thr, 6) == want
        assert ar.class_from_taps(1.0, 0, ar.luma(cols[0]), inside, ids, ar.luma(cols), thr, 6) == want


@functools.lru_cache(maxsize=None)
def _cover_cpu(oracle, w, h, spp, bounces=4):
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam, win = brt.cover_camera(w, h, spp, bounces)
    frame, _ = oracle.render(b, lvl, cam, win, w, h)
    frame.setflags(write=False)
    return b, frame, dr.guides(oracle, b, cam, w, h)


@pytest.mark.parametrize("size", [(33, 17), (64, 40)], ids=lambda s: "%dx%d" % s)
def test_restatement_properties_on_an_oracle_frame(oracle, size):
    w, h = size
    b, base, g = _cover_cpu(oracle, w, h, 2)
    sky = ~(g[..., 3] < np.inf)
    mask = ar.class_mask(base, g, brt.ADAPT_DEFAULT_THRESHOLD, 6)
    sel = mask != 0
    assert sel.any() and (~sel).any() and sky.any()           # (the GPU frame test relies on both kinds at these sizes)
    assert not mask[sky].any()
    huge = ar.class_mask(base, g, 1e30, 6)
    assert not (huge == ar.NOISY).any() and np.array_equal(huge == ar.SPARSE, mask == ar.SPARSE) and (huge == ar.SPARSE).any()
    assert not ar.class_mask(base, g, 1e30, 1).any()          # every classed pixel counts itself
    # the mask is a function of the f32 base frame: whatever format the frame is stored in, it is the same mask
    _, full, _ = _cover_cpu(oracle, w, h, 8)
    for fmt in ("srgb8", "f16", "unorm8"):
        got = ar.adaptive(oracle.encode_frame(base, fmt), oracle.encode_frame(full, fmt), mask)
        assert np.array_equal(got[sel], oracle.encode_frame(full, fmt)[sel]) and np.array_equal(got[~sel], oracle.encode_frame(base, fmt)[~sel])
    print(f"cover {w}x{h} base 2 spp: sparse {int((mask == 1).sum())}, noisy {int((mask == 2).sum())}, sky {int(sky.sum())} of {w * h}")


def test_restatement_single_pixel_frames(oracle):
    b = make_buffers([((0.0, 0.0, -3.0), 1.0, brt.StandardMaterial(base_color=(0.8, 0.3, 0.2)))])
    lvl, cam, win = uniforms(1, 1, 2, 4, (0.0, 0.0, 0.0), (0.0, 0.0, -3.0), 0.9, 0.5)
    base, _ = oracle.render(b, lvl, cam, win, 1, 1)
    g = dr.guides(oracle, b, cam, 1, 1)
    assert g[0, 0, 3] < np.inf and ar.class_mask(base, g, 0.5, 6)[0, 0] == ar.SPARSE      # one tap < min_taps
    lvl, cam, win = uniforms(1, 1, 2, 4, (0.0, 0.0, 0.0), (0.0, 0.0, 3.0), 0.9, 0.5)
    assert ar.class_mask(oracle.render(b, lvl, cam, win, 1, 1)[0], dr.guides(oracle, b, cam, 1, 1), 0.5, 6)[0, 0] == 0      # sky


def test_restatement_quality_bar(oracle):
    """Cover scene, 96x54, 8 bounces, base 8 spp, full 64 spp, on the oracle, against 1024 spp of another window seed: per threshold of
    GRID the selected share s, the samples spent per pixel 8 + 64 s and R = MSE(adaptive) / MSE(uniform at ceil(8 + 64 s) spp).  Asserted:
    R at the default threshold <= 1.1 x the recorded 0.8862, and < 1."""
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    w, h = 96, 54
    lvl, cam_r, win_r = brt.cover_camera(w, h, 1024, 8, brt.Raytracing.Pure, 0.25)
    ref, _ = oracle.render(b, lvl, cam_r, win_r, w, h)
    g = dr.guides(oracle, b, cam_r, w, h)

    @functools.lru_cache(maxsize=None)
    def frame(spp):
        return oracle.render(b, *brt.cover_camera(w, h, spp, 8, brt.Raytracing.Pure, 0.5), w, h)[0]

    base, full = frame(8), frame(64)
    ratios = {}
    for thr in GRID:
        mask = ar.class_mask(base, g, thr, 6)
        s = float((mask != 0).mean())
        k = math.ceil(8 + 64 * s)
        ratios[thr] = ar.mse(ar.adaptive(base, full, mask), ref) / ar.mse(frame(k), ref)
        print(f"threshold {thr:g}: sparse {int((mask == 1).sum())}, noisy {int((mask == 2).sum())}, share {s:.4f}, spent {8 + 64 * s:.2f} spp, "
              f"uniform {k} spp, R {ratios[thr]:.4f}")
    assert brt.ADAPT_DEFAULT_THRESHOLD in GRID and ratios[brt.ADAPT_DEFAULT_THRESHOLD] == min(ratios.values()), ratios
    assert ratios[brt.ADAPT_DEFAULT_THRESHOLD] <= BAR, ratios


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out_tensor(w, h, out_format=brt.FLAG_OUT_RGBA32F, fill=0):
    import torch
    return torch.full((h, w * brt.OUT_PIXEL_BYTES[out_format] // 4), fill, dtype=torch.int32, device="cuda")


def _host(t, h, w):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint8).reshape(h, w, -1)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _bytes(oracle, frame, fmt, h, w):
    f = frame if FORMATS[fmt] is None else oracle.encode_frame(frame, FORMATS[fmt])
    return np.ascontiguousarray(f).view(np.uint8).reshape(h, w, -1)


def _mask(plugin, cam, win, w, h, base, stream=None):
    import torch
    d_base = _device(base)
    m = torch.full((h, w), 0x55, dtype=torch.uint8, device="cuda")
    plugin.node.adaptive_mask_device(cam, win, w, h, d_base.data_ptr(), m.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return m.cpu().numpy()


def _refine(plugin, cam, win, w, h, base, fmt=brt.FLAG_OUT_RGBA32F, stream=None):
    """(frame bytes (h, w, -1) u8, the device count word)"""
    import torch
    d_base, out = _device(base), _out_tensor(w, h, fmt, 0x11111111)
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    plugin.node.adaptive_refine_device(cam, win, w, h, d_base.data_ptr(), out.data_ptr(), count.data_ptr(), stream=stream, out_format=fmt)
    return _host(out, h, w), int(count.cpu()[0])


def _one_call(plugin, cam, win, w, h, fmt=brt.FLAG_OUT_RGBA32F, stream=None):
    import torch
    out = _out_tensor(w, h, fmt, 0x11111111)
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    plugin.node.render_adaptive_device(cam, win, w, h, out.data_ptr(), count.data_ptr(), stream=stream, out_format=fmt)
    return _host(out, h, w), int(count.cpu()[0])


@pytest.fixture
def adaptive(plugin):
    """The tests' settings (base 2 spp of a full 8, the default threshold and min_taps); the library's defaults again afterwards."""
    plugin.set_adaptive(2, brt.ADAPT_DEFAULT_THRESHOLD, 6)
    yield plugin
    plugin.set_adaptive(*DEFAULTS)
    plugin.set_policy(0)


SIZES = [(1, 1), (5, 3), (33, 17), (64, 40)]
CASES = {"cover": (brt.SCENE_COVER, brt.cover_camera), "rtiow": (brt.SCENE_RTIOW_FINAL, brt.rtiow_camera),
         "stress": (brt.SCENE_STRESS_GRID, brt.cover_camera)}


def _view(case, w, h):
    kind, camera = CASES[case]
    lvl, cam2, win = camera(w, h, 2, 4)
    _, cam8, _ = camera(w, h, 8, 4)
    return brt.generate_scene(kind, 1), lvl, cam2, cam8, win


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", list(CASES))
def test_mask_equals_the_restatement(adaptive, case, size):
    """From the GPU's own base frame and guides, tolerance 0; at the default threshold and at one that leaves hit pixels unselected."""
    plugin, (w, h) = adaptive, size
    b, lvl, cam2, cam8, win = _view(case, w, h)
    base = plugin.node.run(lvl, cam2, win, w, h, buffers=b).copy()
    g = plugin.debug_denoise_guides(cam8, win, w, h)
    for thr, mt in ((brt.ADAPT_DEFAULT_THRESHOLD, 6), (0.4, 6), (0.4, 25), (0.1, 1)):
        plugin.set_adaptive(2, thr, mt)
        want = ar.class_mask(base, g, thr, mt)
        got = _mask(plugin, cam8, win, w, h, base)
        assert np.array_equal(got, want), (case, size, thr, mt, int((got != want).sum()))
        _, count = _refine(plugin, cam8, win, w, h, base)
        assert count == int((want != 0).sum()), (case, size, thr, mt)
        print(f"{case} {w}x{h} threshold {thr:g} min_taps {mt}: sparse {int((want == 1).sum())}, noisy {int((want == 2).sum())} of {w * h}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", list(CASES))
def test_frame_equals_the_oracle_under_the_gpus_own_mask(adaptive, oracle, case, size):
    """Selected pixels: the oracle's 8-spp frame; the rest: its 2-spp frame; in all four store formats and both pixel-tracer forms."""
    plugin, (w, h) = adaptive, size
    b, lvl, cam2, cam8, win = _view(case, w, h)
    base, _ = oracle.render(b, lvl, cam2, win, w, h)
    full, _ = oracle.render(b, lvl, cam8, win, w, h)
    plugin.node.write_buffers(b)
    one, n_one = _one_call(plugin, cam8, win, w, h)
    if case == "stress":
        assert plugin.node.last_stats["scene_in_lds"] == 2, plugin.node.last_stats       # the top of the tree in LDS
    mask = _mask(plugin, cam8, win, w, h, base)
    sel = mask != 0
    if case == "cover" and w >= 33:
        assert sel.any() and (~sel).any()
    assert n_one == int(sel.sum())
    for fmt in FORMATS:
        want = ar.adaptive(_bytes(oracle, base, fmt, h, w), _bytes(oracle, full, fmt, h, w), mask)
        for form in (0, 1):
            with plugin.tuning(BRT_PIXELS_FORM=form):
                got, count = _refine(plugin, cam8, win, w, h, base, fmt)
            assert count == int(sel.sum()), (case, size, fmt, form)
            assert _same_bits(got[sel], want[sel]), (case, size, fmt, form, "selected")
            assert _same_bits(got[~sel], want[~sel]), (case, size, fmt, form, "base")
    assert _same_bits(one, ar.adaptive(_bytes(oracle, base, brt.FLAG_OUT_RGBA32F, h, w), _bytes(oracle, full, brt.FLAG_OUT_RGBA32F, h, w), mask))


@pytest.fixture(scope="module")
def cover(oracle):
    """Cover scene 64x40, 4 bounces: the oracle's 2-spp and 8-spp frames, shared and never written."""
    w, h = 64, 40
    b, lvl, cam2, cam8, win = _view("cover", w, h)
    base, _ = oracle.render(b, lvl, cam2, win, w, h)
    full, _ = oracle.render(b, lvl, cam8, win, w, h)
    base.setflags(write=False)
    full.setflags(write=False)
    return b, lvl, cam2, cam8, win, base, full


@pytest.mark.gpu
def test_edge_settings(adaptive, cover, oracle):
    plugin = adaptive
    b, lvl, cam2, cam8, win, base, full = cover
    w, h = 64, 40
    plugin.node.write_buffers(b)
    g = plugin.debug_denoise_guides(cam8, win, w, h)
    hit = g[..., 3] < np.inf
    plugin.set_adaptive(2, 1e30, 1)                     # nothing can be selected: the base frame bitwise
    for fmt in (brt.FLAG_OUT_RGBA32F, brt.FLAG_OUT_RGBA16F):
        got, count = _one_call(plugin, cam8, win, w, h, fmt)
        assert count == 0 and _same_bits(got, _refine(plugin, cam8, win, w, h, base, fmt)[0])
    assert _same_bits(_one_call(plugin, cam8, win, w, h)[0].view(F32), base)
    assert not _mask(plugin, cam8, win, w, h, base).any()
    plugin.set_adaptive(2, 1e-30, 6)                    # every hit pixel of a noisy frame: bitwise the full frame there
    got, count = _one_call(plugin, cam8, win, w, h)
    mask = _mask(plugin, cam8, win, w, h, base)
    assert np.array_equal(mask != 0, ar.class_mask(base, g, 1e-30, 6) != 0) and not mask[~hit].any()
    assert count == int((mask != 0).sum()) > 0.9 * hit.sum()
    assert _same_bits(got.view(F32)[mask != 0], full[mask != 0]) and _same_bits(got.view(F32)[mask == 0], base[mask == 0])
    full_srgb = _bytes(oracle, full, brt.FLAG_OUT_RGBA8_UNORM_SRGB, h, w)
    for spp in (8, 9, 65535):                           # base_spp >= sample_count: the plain frame, nothing selected
        plugin.set_adaptive(spp, brt.ADAPT_DEFAULT_THRESHOLD, 6)
        got, count = _one_call(plugin, cam8, win, w, h, brt.FLAG_OUT_RGBA8_UNORM_SRGB)
        assert count == 0 and _same_bits(got, full_srgb), spp
        assert not _mask(plugin, cam8, win, w, h, base).any()
        got, count = _refine(plugin, cam8, win, w, h, full)
        assert count == 0 and _same_bits(got.view(F32), full)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [brt.FLAG_OUT_RGBA32F, brt.FLAG_OUT_RGBA8_UNORM_SRGB], ids=["f32", "srgb8"])
def test_one_call_equals_its_steps(adaptive, cover, fmt):
    import torch
    plugin = adaptive
    b, lvl, cam2, cam8, win, base, full = cover
    w, h = 64, 40
    plugin.node.write_buffers(b)
    d_base = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    plugin.node.render_device(lvl, cam2, win, w, h, d_base.data_ptr())
    base_rays = plugin.node.last_stats["rays"]
    assert _same_bits(d_base.cpu().numpy(), base)
    steps, n_steps = _refine(plugin, cam8, win, w, h, d_base.cpu().numpy(), fmt)
    one, n_one = _one_call(plugin, cam8, win, w, h, fmt)
    st = plugin.node.last_stats
    mask = _mask(plugin, cam8, win, w, h, base)
    assert _same_bits(one, steps) and n_one == n_steps == int((mask != 0).sum()) > 0
    assert st["paths"] == w * h * 2 and st["total_ms"] > 0 and st["rays"] > base_rays       # base plus re-trace


@pytest.mark.gpu
def test_scene_of_32_bit_descriptors(adaptive, oracle):
    plugin = adaptive
    w, h = 64, 40
    lvl, cam2, win = big_view(w, h, spp=2)
    _, cam8, _ = big_view(w, h, spp=8)
    b32, win, st = resident_callee_tree(plugin, big_scene(16383, 7), lvl, cam2, win, w, h)
    base, _ = oracle.render(b32, lvl, cam2, win, w, h)
    full, _ = oracle.render(b32, lvl, cam8, win, w, h)
    plugin.set_adaptive(2, 0.4, 6)
    got, count = _one_call(plugin, cam8, win, w, h)
    st = plugin.node.last_stats
    print(f"n = 16383: scene_in_lds {st['scene_in_lds']}, hot_records {st['hot_records']}, kernel_variant {st['kernel_variant']}")
    assert st["scene_in_lds"] == 0 and st["hot_records"] == 0, st                            # 32-bit descriptors: walked from global memory
    mask = _mask(plugin, cam8, win, w, h, base)
    assert np.array_equal(mask, ar.class_mask(base, plugin.debug_denoise_guides(cam8, win, w, h), 0.4, 6))
    assert 0 < count == int((mask != 0).sum()) < w * h
    assert _same_bits(got.view(F32), ar.adaptive(base, full, mask))


@pytest.mark.gpu
def test_plain_frames_and_the_dispatch_history_do_not_change(adaptive, oracle):
    """64 spp with base 8 (a pre-pass runs from 32 spp on): plain frame, adaptive frames, plain frame.  The plain frames and their ray
    counts are equal; no adaptive call of a still view runs a pre-pass (the base trace shares the view's order, which is keyed on the
    frame's size, not its sample count); the ray-count history of the plain frames is kept apart from the base frames'."""
    import torch
    plugin = adaptive
    w, h = 64, 40
    b = brt.generate_scene(brt.SCENE_COVER, 1)
    lvl, cam64, win = brt.cover_camera(w, h, 64, 4)
    plugin.set_adaptive(*DEFAULTS)
    frame = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    fresh = brt.RaytracePlugin([0])
    try:
        fresh.set_adaptive(*DEFAULTS)
        fresh.node.write_buffers(b)
        fresh.node.render_device(lvl, cam64, win, w, h, frame.data_ptr())
        fresh.node.render_device(lvl, cam64, win, w, h, frame.data_ptr())
        first, st_first = frame.cpu().numpy(), dict(fresh.node.last_stats)
        stats = []
        for _ in range(4):
            out, _ = _one_call(fresh, cam64, win, w, h)
            stats.append(dict(fresh.node.last_stats))
        fresh.node.render_device(lvl, cam64, win, w, h, frame.data_ptr())
        again, st_again = frame.cpu().numpy(), dict(fresh.node.last_stats)
    finally:
        fresh.close()
    assert _same_bits(first, again) and st_first["rays"] == st_again["rays"] and st_first["paths"] == st_again["paths"]
    assert st_again["prepass_ms"] == 0 and st_again["kernel_variant"] == st_first["kernel_variant"], (st_first, st_again)
    assert all(s["prepass_ms"] == 0 for s in stats[2:]), [s["prepass_ms"] for s in stats]
    assert all(s["rays"] == stats[0]["rays"] and s["paths"] == w * h * 8 for s in stats)
    full, _ = oracle.render(b, lvl, cam64, win, w, h)
    assert _same_bits(first, full)


@pytest.mark.gpu
def test_caller_streams_and_two_calls_in_flight(adaptive, cover, oracle):
    import torch
    plugin = adaptive
    b, lvl, cam2, cam8, win, base, full = cover
    w, h = 64, 40
    plugin.node.write_buffers(b)
    mask = _mask(plugin, cam8, win, w, h, base)
    want = ar.adaptive(base, full, mask)
    win_b = brt.WindowExtract.extract_component(h, 0.25)
    base_b, _ = oracle.render(b, lvl, cam2, win_b, w, h)
    full_b, _ = oracle.render(b, lvl, cam8, win_b, w, h)
    want_b = ar.adaptive(base_b, full_b, _mask(plugin, cam8, win_b, w, h, base_b))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    out_a, out_b = _out_tensor(w, h), _out_tensor(w, h)
    n_a = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    n_b = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        torch.cuda._sleep(20_000_000)                   # (a few ms: A's kernels start after B's calls have been made)
    st = plugin.node.render_adaptive_device(cam8, win, w, h, out_a.data_ptr(), n_a.data_ptr(), stream=sa.cuda_stream)
    assert st["rays"] == 0                              # a caller's stream: the call does not synchronise
    plugin.node.render_adaptive_device(cam8, win_b, w, h, out_b.data_ptr(), n_b.data_ptr(), stream=sb.cuda_stream)
    d_base = _device(base)
    out_c = _out_tensor(w, h)
    with torch.cuda.stream(sa):
        plugin.node.adaptive_refine_device(cam8, win, w, h, d_base.data_ptr(), out_c.data_ptr(), stream=sa.cuda_stream)
    torch.cuda.synchronize()
    assert _same_bits(_host(out_a, h, w).view(F32), want) and int(n_a.cpu()[0]) == int((mask != 0).sum())
    assert _same_bits(_host(out_b, h, w).view(F32), want_b)
    assert _same_bits(_host(out_c, h, w).view(F32), want)
    assert _same_bits(_one_call(plugin, cam8, win, w, h)[0].view(F32), want)               # and the own stream afterwards


@pytest.mark.gpu
def test_larger_frames_behind_a_held_one_grow_the_buffers(adaptive, cover, oracle):
    """A 32x20 frame is held on stream A of a new context; 64x40 frames follow on stream B and on the context's own stream with no host
    synchronisation in between.  They need a larger list (d_pxbuf), base frame (d_uplow) and denoise scratch, each of which is
    reallocated only behind the held frame's last use of it.  All three frames are the expected ones; the held one is read last."""
    import torch
    plugin = adaptive
    b, lvl, cam2, cam8, win, base, full = cover
    w, h, ws, hs = 64, 40, 32, 20
    plugin.node.write_buffers(b)
    mask = _mask(plugin, cam8, win, w, h, base)
    want = ar.adaptive(base, full, mask)
    _, cam2s, wins = brt.cover_camera(ws, hs, 2, 4)
    _, cam8s, _ = brt.cover_camera(ws, hs, 8, 4)
    base_s, _ = oracle.render(b, lvl, cam2s, wins, ws, hs)
    full_s, _ = oracle.render(b, lvl, cam8s, wins, ws, hs)
    mask_s = _mask(plugin, cam8s, wins, ws, hs, base_s)
    want_s = ar.adaptive(base_s, full_s, mask_s)
    assert (mask_s != 0).any() and (mask_s == 0).any()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    out_a, out_b, out_c = _out_tensor(ws, hs, fill=0x11111111), _out_tensor(w, h, fill=0x11111111), _out_tensor(w, h, fill=0x11111111)
    n_a = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    n_b = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    fresh = brt.RaytracePlugin([0])
    try:
        fresh.set_adaptive(2, brt.ADAPT_DEFAULT_THRESHOLD, 6)
        fresh.node.write_buffers(b)
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(20_000_000)                   # (a few ms: A's kernels start after the later calls have been made)
        fresh.node.render_adaptive_device(cam8s, wins, ws, hs, out_a.data_ptr(), n_a.data_ptr(), stream=sa.cuda_stream)
        fresh.node.render_adaptive_device(cam8, win, w, h, out_b.data_ptr(), n_b.data_ptr(), stream=sb.cuda_stream)
        fresh.node.render_adaptive_device(cam8, win, w, h, out_c.data_ptr())
        torch.cuda.synchronize()
        assert _same_bits(_host(out_b, h, w).view(F32), want) and int(n_b.cpu()[0]) == int((mask != 0).sum())
        assert _same_bits(_host(out_c, h, w).view(F32), want)
        assert _same_bits(_host(out_a, hs, ws).view(F32), want_s) and int(n_a.cpu()[0]) == int((mask_s != 0).sum())
    finally:
        fresh.close()


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(adaptive, cover):
    import torch
    plugin = adaptive
    b, lvl, cam2, cam8, win, base, full = cover
    w, h = 64, 40
    plugin.node.write_buffers(b)
    lib, ctx = plugin._lib, plugin._ctx
    for bad in ((0, 0.5, 6), (65536, 0.5, 6), (8, 0.0, 6), (8, -1.0, 6), (8, float("inf"), 6), (8, float("nan"), 6), (8, 0.5, 0), (8, 0.5, 26)):
        assert lib.brt_set_adaptive(ctx, *bad) == ERR_INVALID, bad
    d_base, out = _device(base), _out_tensor(w, h)
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    c, wn = cam8.ctypes.data, win.ctypes.data

    def one(flags=0, o=out.data_ptr(), cam_p=c, sizes=(w, h)):
        return lib.brt_render_adaptive_device(ctx, cam_p, wn, sizes[0], sizes[1], o, None, None, flags, None)

    def refine(flags=0, o=out.data_ptr(), lo=d_base.data_ptr(), cam_p=c, sizes=(w, h)):
        return lib.brt_adaptive_refine_device(ctx, cam_p, wn, sizes[0], sizes[1], lo, o, None, None, flags, None)

    def maskf(flags=0, m=mask.data_ptr(), lo=d_base.data_ptr(), cam_p=c):
        return lib.brt_adaptive_mask_device(ctx, cam_p, wn, w, h, lo, m, None, flags)

    for flags in (brt.FLAG_DENOISE, brt.FLAG_TEMPORAL, brt.FLAG_DENOISE | brt.FLAG_TEMPORAL, brt.FLAG_KERNEL_SIMPLE, brt.FLAG_BLEND_POST,
                  brt.FLAG_COUNTERS, 1 << 30):
        assert one(flags) == ERR_INVALID and refine(flags) == ERR_INVALID and maskf(flags) == ERR_INVALID, flags
    assert maskf(brt.FLAG_OUT_RGBA16F) == ERR_INVALID
    assert refine(o=d_base.data_ptr()) == ERR_INVALID and maskf(m=d_base.data_ptr()) == ERR_INVALID       # overlapping buffers
    assert one(o=None) == ERR_INVALID and refine(o=None) == ERR_INVALID and refine(lo=None) == ERR_INVALID and maskf(m=None) == ERR_INVALID
    assert one(cam_p=None) == ERR_INVALID and refine(cam_p=None) == ERR_INVALID and maskf(cam_p=None) == ERR_INVALID
    for sizes in ((0, h), (w, 0), (32769, h), (w, 32769)):
        assert one(sizes=sizes) == ERR_INVALID and refine(sizes=sizes) == ERR_INVALID, sizes
    ortho = cam8.copy()
    ortho["projection"] = 1
    assert one(cam_p=ortho.ctypes.data) == ERR_UNSUPPORTED and refine(cam_p=ortho.ctypes.data) == ERR_UNSUPPORTED
    assert maskf(cam_p=ortho.ctypes.data) == ERR_UNSUPPORTED
    plugin.set_policy(brt.POLICY_OR_SHORT_CIRCUIT)
    try:
        assert one() == ERR_UNSUPPORTED and refine() == ERR_UNSUPPORTED and maskf() == ERR_UNSUPPORTED
    finally:
        plugin.set_policy(0)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any() and not mask.cpu().numpy().any()
    fresh = brt.RaytracePlugin([0])
    try:
        assert fresh._lib.brt_render_adaptive_device(fresh._ctx, c, wn, w, h, out.data_ptr(), None, None, 0, None) == ERR_NO_SCENE
        assert fresh._lib.brt_adaptive_refine_device(fresh._ctx, c, wn, w, h, d_base.data_ptr(), out.data_ptr(), None, None, 0, None) == ERR_NO_SCENE
        assert fresh._lib.brt_adaptive_mask_device(fresh._ctx, c, wn, w, h, d_base.data_ptr(), mask.data_ptr(), None, 0) == ERR_NO_SCENE
    finally:
        fresh.close()
    got, count = _one_call(plugin, cam8, win, w, h)                                        # the settings and the context are as they were
    m = _mask(plugin, cam8, win, w, h, base)
    assert count == int((m != 0).sum()) > 0 and _same_bits(got.view(F32), ar.adaptive(base, full, m))
