"""k_upscale (brt_upscale.hip) on low frames the tracer never renders (tests/upscale_synth.py) and at edge size pairs: the finite3
rejections of tap() and of stage C, stage B's gather at the frame border, stage C, the (0, 0, 0, 1) store, one-row and one-column frames,
a one-pixel low frame, ratio 1 and just above 1, the 32768 maximum, the sigmas of brt_set_denoise, and the select / mask and blended
forms on the same frames.  References: the f32 restatement (tests/upscale_ref.py), a float64 evaluation of the rule
(tests/upscale_ref64.py), the oracle's encoders and the plain kernel's own output.  No stage count is taken from the kernel.

CPU: every generator's non-vacuity condition at every size pair it is used at (guides from the oracle's raycast), and the restatement
against the float64 reference on every frame and pair, and at every sigma pair, to DESIGN section 14's 1e-4 max(1, |ref|) (`-rP`
prints the largest error per pattern; the table is in DESIGN section 14).  No sigma pair exceeds the bound, none is dropped.

Finding (docs/experiments.md, "Upsampling a finite 3e38"): the `overflow` frame at 65x37 from 17x10 and at 40x24 from 39x23 has one
output pixel on a refracting sphere (a = 1, so 3e38 / a is finite and the tap eligible) whose stage A weight is above 1.134: w c'
passed FLT_MAX and the f32 rule stored +Inf where the float64 rule gives 3e38.  The stage weights are now scaled by powers of two
(kUpscaleScaleA / B / C), which keeps every sum finite and every other result's bits.  Second finding: test_store_formats_on_blocks2
at 64x36 from 32x18 met an f32 result on an f16 tie, where the RGBA16F instantiations' fused multiply-and-convert (v_fma_mixlo_f16)
rounded once and not twice; the kernel now keeps the product an f32 value before the store."""
import functools

import numpy as np
import pytest

import bevyray_amd as brt
import denoise_ref as dr
import upscale_blend_ref as ubr
import upscale_ref as ur
import upscale_ref64 as u64
import upscale_refine_ref as rr
import upscale_synth as sy
from helpers import uniforms

F32 = np.float32
BOUND = 1e-4                        # |got - ref| <= 1e-4 max(1, |ref|)
GUARD = 0x11111111
FORMATS = ((brt.FLAG_OUT_RGBA32F, None), (brt.FLAG_OUT_RGBA8_UNORM_SRGB, "srgb8"), (brt.FLAG_OUT_RGBA8_UNORM, "unorm8"),
           (brt.FLAG_OUT_RGBA16F, "f16"))
SIGMA_PAIRS = [(sn, sz) for sn in (1e-3, 1.0, 128.0, 4096.0) for sz in (1e-3, 1.0, 1e3)]      # (sigma_normal, sigma_depth); none dropped
SIGMA_IDS = ["n%g_z%g" % p for p in SIGMA_PAIRS]
STRESS_PAIR = sy.PAIRS[0]
COVER_VIEW = dict(pos=(13.0, 2.0, 3.0), target=(0.0, 0.0, 0.0), fov=0.4, up=(0.0, 1.0, 0.0))          # brt.cover_camera's
# the ground sphere's horizon from the cover camera's position; the row view is rolled by 45 degrees, so that a one-row frame crosses it
COLUMN_VIEW = dict(pos=(13.0, 2.0, 3.0), target=(0.0, 1.2, 0.0), fov=0.4, up=(0.0, 1.0, 0.0))
ROW_VIEW = dict(pos=(13.0, 2.0, 3.0), target=(0.0, 1.2, 0.0), fov=0.4, up=(0.0, 1.0, 1.0))
EDGE_PAIRS = [((48, 1, 12, 1), ROW_VIEW), ((1, 48, 1, 12), COLUMN_VIEW), ((4, 4, 1, 1), COVER_VIEW), ((16, 16, 16, 16), COVER_VIEW),
              ((15, 17, 15, 17), COVER_VIEW), ((17, 15, 5, 4), COVER_VIEW), ((33, 31, 9, 8), COVER_VIEW), ((40, 24, 39, 23), COVER_VIEW),
              ((32768, 1, 8192, 1), ROW_VIEW), ((1, 32768, 1, 8192), COLUMN_VIEW)]
REFINE_PAIRS = [(96, 54, 48, 27), (17, 15, 5, 4)]


def _pairs_of(pattern):
    return sy.BLOCKS6_PAIRS if pattern == "blocks6" else sy.PAIRS


@functools.lru_cache(maxsize=None)
def _scene(kind):
    return brt.generate_scene(kind, 1)


def _view(pair, spp=2, bounces=4):
    """(level, camera, window, low window) of the cover view at the pair's full size."""
    w, h, lw, lh = pair
    lvl, cam, win = brt.cover_camera(w, h, spp, bounces)
    return lvl, cam, win, brt.upscale_window(win, h, lh)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cpu_guides(oracle, kind, pair):
    """(camera, low guides, full guides) from the oracle's raycast: shared, never written."""
    w, h, lw, lh = pair
    _, cam, _, _ = _view(pair)
    g_low, g_full = dr.guides(oracle, _scene(kind), cam, lw, lh), dr.guides(oracle, _scene(kind), cam, w, h)
    g_low.setflags(write=False)
    g_full.setflags(write=False)
    return cam, g_low, g_full


CONDITION_CASES = [(brt.SCENE_COVER, pattern, pair) for pattern in sy.PATTERNS for pair in _pairs_of(pattern)]
CONDITION_CASES += [(brt.SCENE_STRESS_GRID, pattern, STRESS_PAIR) for pattern in sy.PATTERNS]


@pytest.mark.parametrize("kind,pattern,pair", CONDITION_CASES,
                         ids=["%s-%s-%s" % ("stress" if k else "cover", p, sy.pair_id(s)) for k, p, s in CONDITION_CASES])
def test_generators_meet_their_conditions(oracle, kind, pattern, pair):
    cam, g_low, g_full = _cpu_guides(oracle, kind, pair)
    low = sy.frame(pattern, g_low)
    out, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
    counts = sy.check_conditions(pattern, stage, pair)
    print(f"{pattern} {sy.pair_id(pair)}: sky / A / B / C / none {counts}")
    assert counts[ur.SKY] >= sy.MIN_PIXELS                                  # (and both hit and sky pixels, as every frame here)
    assert np.array_equal(low[..., 3], np.ones_like(low[..., 3])) or pattern == "alpha_junk"
    assert np.isfinite(out).all()                   # whatever the low frame holds: only finite taps are read and no sum overflows
    if pattern == "blocks2":                        # all five outcomes, at every pair
        assert min(counts) >= sy.MIN_PIXELS, counts
    if pattern == "signs_and_small":
        c = low[..., :3]
        assert (c < 0).any() and np.signbit(c[c == 0]).any() and ((c > 0) & (c < np.finfo(F32).tiny)).any()
        assert (c == F32(1e-30)).any() and (c == F32(1e30)).any()
    if pattern == "overflow":
        big = low[..., 0] == F32(sy.OVERFLOW)
        with np.errstate(over="ignore"):
            assert big.any() and not np.isfinite(low[big][:, :3] / g_low[big][:, 4:7]).all()


def test_finite_taps_give_a_finite_pixel(oracle):
    """The two pairs at which the `overflow` frame has a 3e38 tap that stays eligible (a = 1: a refracting sphere) under a stage A weight
    above FLT_MAX / 3e38 = 1.134 before the scaling of the weights: the f32 rule gave +Inf there, float64 3e38."""
    for pair in (sy.PAIRS[1], sy.PAIRS[3]):
        cam, g_low, g_full = _cpu_guides(oracle, brt.SCENE_COVER, pair)
        low = sy.frame("overflow", g_low)
        hit_low = g_low[..., 3] < np.inf
        assert (hit_low & (low[..., 0] == F32(sy.OVERFLOW)) & (g_low[..., 4] == 1)).any()          # an eligible 3e38 tap
        out, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
        want, _ = u64.upscale_frame(oracle, low, g_low, g_full, cam)
        big = (want[..., :3] > 1e38).all(-1) & (stage == ur.STAGE_A)
        assert big.any() and np.isfinite(out).all()
        assert np.abs(out[big][:, :3] / want[big][:, :3] - 1.0).max() <= BOUND


def test_scaling_the_weights_keeps_the_bits(oracle):
    """The powers of two of kUpscaleScaleA / B / C scale every product and sum exactly: on frames with no denormal product (every
    pattern but `signs_and_small`, and a frame of ordinary values) the restatement with and without them is the same bit for bit,
    but for the `overflow` pixels the scaling is there for, which were +Inf."""
    for pair in sy.PAIRS:
        cam, g_low, g_full = _cpu_guides(oracle, brt.SCENE_COVER, pair)
        for name in ("random",) + tuple(p for p in sy.PATTERNS if p != "signs_and_small" and pair in _pairs_of(p)):
            low = sy.base_frame(g_low, 9) if name == "random" else sy.frame(name, g_low)
            new, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
            old, stage_old = ur.upscale_frame(oracle, low, g_low, g_full, cam, scales=(1.0, 1.0, 1.0))
            assert np.array_equal(stage, stage_old)
            same = np.isfinite(old).all(-1)
            assert same.all() or name == "overflow", (pair, name)
            assert np.array_equal(new[same].view(np.uint32), old[same].view(np.uint32)), (pair, name)
            assert np.isfinite(new).all()


@pytest.mark.parametrize("pattern", sy.PATTERNS)
def test_restatement_against_float64(oracle, pattern):
    """Every synthetic frame at every pair it is used at: equal stages, finite float64 results within the bound, the same class where
    the float64 result is not finite."""
    worst = 0.0
    for pair in _pairs_of(pattern):
        cam, g_low, g_full = _cpu_guides(oracle, brt.SCENE_COVER, pair)
        low = sy.frame(pattern, g_low)
        got, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
        want, stage64 = u64.upscale_frame(oracle, low, g_low, g_full, cam)
        assert np.array_equal(stage, stage64), (pattern, pair, int((stage != stage64).sum()))
        err, same_class = u64.compare(got, want)
        print(f"{pattern} {sy.pair_id(pair)}: max |f32 - f64| / max(1, |f64|) = {err:.3g}")
        assert same_class and err <= BOUND, (pattern, pair, err)
        worst = max(worst, err)
    print(f"{pattern}: largest over the pairs {worst:.3g}")


def test_alpha_junk_is_checker(oracle):
    for pair in sy.PAIRS:
        cam, g_low, g_full = _cpu_guides(oracle, brt.SCENE_COVER, pair)
        junk, plain = sy.frame("alpha_junk", g_low), sy.frame("checker", g_low)
        assert np.array_equal(junk[..., :3].view(np.uint32), plain[..., :3].view(np.uint32)) and not np.isfinite(junk[..., 3]).all()
        a, sa = ur.upscale_frame(oracle, junk, g_low, g_full, cam)
        b, sb = ur.upscale_frame(oracle, plain, g_low, g_full, cam)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(sa, sb)
        c, _ = u64.upscale_frame(oracle, junk, g_low, g_full, cam)
        d, _ = u64.upscale_frame(oracle, plain, g_low, g_full, cam)
        assert np.array_equal(c, d)


@pytest.mark.parametrize("sigmas", SIGMA_PAIRS, ids=SIGMA_IDS)
def test_restatement_against_float64_at_sigma_pairs(oracle, sigmas):
    """pow(nd, sigma_n) exp(-dz) in f32 against float64 on the `checker` frame at 64x36 from 32x18.  Measured: at most 3.9e-5 (4096 /
    1e3); no pair is above the bound, so none is dropped from the GPU list."""
    sn, sz = sigmas
    cam, g_low, g_full = _cpu_guides(oracle, brt.SCENE_COVER, sy.PAIRS[0])
    low = sy.frame("checker", g_low)
    got, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam, sigma_n=sn, sigma_z=sz)
    want, stage64 = u64.upscale_frame(oracle, low, g_low, g_full, cam, sigma_n=sn, sigma_z=sz)
    err, same_class = u64.compare(got, want)
    print(f"sigma_normal {sn:g} sigma_depth {sz:g}: max |f32 - f64| / max(1, |f64|) = {err:.3g}")
    assert np.array_equal(stage, stage64) and same_class and err <= BOUND, (sigmas, err)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(w, h, fmt):
    import torch
    return torch.full((h + 1, w * brt.OUT_PIXEL_BYTES[fmt] // 4), GUARD, dtype=torch.int32, device="cuda")      # (a guard row behind the frame)


def _frame_of(out, w, h):
    import torch
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[h] == GUARD).all(), "guard row"
    return raw[:h].view(np.uint8).reshape(h, w, -1)


def _upscale(plugin, cam, win, lw, lh, low, w, h, fmt=brt.FLAG_OUT_RGBA32F):
    d_low, out = _device(low), _guarded(w, h, fmt)
    plugin.node.upscale_device(cam, win, lw, lh, d_low.data_ptr(), w, h, out.data_ptr(), out_format=fmt)
    return _frame_of(out, w, h)


def _gpu_guides(plugin, cam, win, pair):
    w, h, lw, lh = pair
    return plugin.debug_denoise_guides(cam, brt.upscale_window(win, h, lh), lw, lh), plugin.debug_denoise_guides(cam, win, w, h)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_against(got, want, stage, what, want64=None):
    """The sky bitwise, the none pixels bitwise (0, 0, 0, 1), everything else within the bound of the f32 restatement (and of the
    float64 reference) with the class of every non-finite channel identical.  -> the largest error against the restatement."""
    sky, none = stage == ur.SKY, stage == ur.STAGE_NONE
    assert _same_bits(got[sky], want[sky]), (what, "sky")
    assert _same_bits(got[none], np.broadcast_to(np.array([0, 0, 0, 1], F32), got[none].shape)), (what, "none")
    assert (got[..., 3] == 1).all(), (what, "alpha")
    err, same_class = u64.compare(got, want)
    assert same_class and err <= BOUND, (what, "f32 restatement", err)
    if want64 is not None:
        err64, same_class = u64.compare(got, want64)
        assert same_class and err64 <= BOUND, (what, "float64 reference", err64)
    return err


def _upload(plugin, case, pair):
    """-> (Buffers, camera, window): the scene of `case` resident, the cover view at the pair's full size."""
    b = _scene(brt.SCENE_STRESS_GRID if case == "stress" else brt.SCENE_COVER)
    lvl, cam, win, lwin = _view(pair)
    buffers = brt.Buffers(b.models, b.materials, None) if case == "cover_callee" else b
    if case == "stress":
        plugin.node.run(lvl, cam, lwin, pair[2], pair[3], buffers=buffers)
        assert plugin.node.last_stats["scene_in_lds"] == 2                 # top of the tree in LDS, the rest from L2
    else:
        plugin.node.write_buffers(buffers)
    return b, cam, win


PLAIN_CASES = [(case, pair) for case in ("cover_callee", "cover_caller") for pair in sy.PAIRS] + [("stress", STRESS_PAIR)]
PLAIN_IDS = ["%s-%s" % (c, sy.pair_id(p)) for c, p in PLAIN_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", sy.PATTERNS)
@pytest.mark.parametrize("case,pair", PLAIN_CASES, ids=PLAIN_IDS)
def test_plain_kernel_on_synthetic_frames(plugin, oracle, case, pair, pattern):
    w, h, lw, lh = pair
    _, cam, win = _upload(plugin, case, pair)
    g_low, g_full = _gpu_guides(plugin, cam, win, pair)
    low = sy.frame(pattern, g_low)
    want, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
    if pair in _pairs_of(pattern):
        sy.check_conditions(pattern, stage, (case, pair))              # on the GPU's own guides
    want64, stage64 = u64.upscale_frame(oracle, low, g_low, g_full, cam)
    assert np.array_equal(stage, stage64)
    got = _upscale(plugin, cam, win, lw, lh, low, w, h).view(F32)
    err = _check_against(got, want, stage, (case, pair, pattern), want64)
    print(f"{case} {sy.pair_id(pair)} {pattern}: max err {err:.3g}, sky / A / B / C / none {sy.stage_counts(stage)}")
    if pattern == "alpha_junk":
        assert _same_bits(got, _upscale(plugin, cam, win, lw, lh, sy.frame("checker", g_low), w, h).view(F32))


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sy.PAIRS, ids=sy.pair_id)
def test_store_formats_on_blocks2(plugin, oracle, pair):
    """The three other store formats are oracle.encode_frame of the f32 output, none pixels and stages B and C included."""
    w, h, lw, lh = pair
    _, cam, win = _upload(plugin, "cover_callee", pair)
    g_low, g_full = _gpu_guides(plugin, cam, win, pair)
    low = sy.frame("blocks2", g_low)
    _, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
    sy.check_conditions("blocks2", stage, pair)
    f32 = _upscale(plugin, cam, win, lw, lh, low, w, h).view(F32)
    for fmt, name in FORMATS[1:]:
        want = oracle.encode_frame(f32, name)
        got = _upscale(plugin, cam, win, lw, lh, low, w, h, fmt).view(want.dtype).reshape(want.shape)
        bad = np.argwhere((got != want).any(-1))
        assert not len(bad), (name, len(bad), [(int(y), int(x), int(stage[y, x]), f32[y, x].tolist(), got[y, x].tolist(), want[y, x].tolist())
                                               for y, x in bad[:4]])


@pytest.mark.gpu
@pytest.mark.parametrize("frame", ["random", "blocks2"])
@pytest.mark.parametrize("pair,view", EDGE_PAIRS, ids=[sy.pair_id(p) for p, _ in EDGE_PAIRS])
def test_edge_size_pairs(plugin, oracle, pair, view, frame):
    w, h, lw, lh = pair
    assert lw <= w <= 4 * lw and lh <= h <= 4 * lh and max(w, h) <= 32768           # within sizes_check
    b = _scene(brt.SCENE_COVER)
    _, cam, win = uniforms(w, h, 2, 4, seed=0.5, **view)
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    g_low, g_full = _gpu_guides(plugin, cam, win, pair)
    hit = g_full[..., 3] < np.inf
    assert hit.any() and (~hit).any(), (int(hit.sum()), hit.size)
    low = sy.base_frame(g_low, 9) if frame == "random" else sy.frame("blocks2", g_low)
    want, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
    want64 = None
    if max(w, h) < 1024:           # the float64 reference takes its floors from float64 positions, which holds below 2^10 pixels or so
        want64, stage64 = u64.upscale_frame(oracle, low, g_low, g_full, cam)       # (upscale_ref64.py): the 32768 pairs have the restatement alone
        assert np.array_equal(stage, stage64)
    got = _upscale(plugin, cam, win, lw, lh, low, w, h).view(F32)
    err = _check_against(got, want, stage, (pair, frame), want64)
    print(f"{sy.pair_id(pair)} {frame}: max err {err:.3g}, sky / A / B / C / none {sy.stage_counts(stage)}")
    if frame == "blocks2":
        assert (stage[hit] != ur.STAGE_A).any()                            # (some footprint is gone, whatever the size)
    if pair == (16, 16, 16, 16) and frame == "random":
        # the restatement's ratio-one property (test_upscale.py): every hit pixel is its own tap at weight 1, the others at 2^-26
        assert (stage[hit] == ur.STAGE_A).all()
        assert np.abs(got[hit][:, :3] - low[hit][:, :3]).max() <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("sigmas", SIGMA_PAIRS, ids=SIGMA_IDS)
def test_sigma_settings(plugin, oracle, sigmas):
    """The kernel's one exp2(sigma_n log2(nd) - dz log2 e) against the restatement's pow(nd, sigma_n) exp(-dz) and against float64, on
    the `checker` frame and on a rendered one."""
    sn, sz = sigmas
    pair = sy.PAIRS[0]
    w, h, lw, lh = pair
    b = _scene(brt.SCENE_COVER)
    lvl, cam, win, lwin = _view(pair)
    rendered = plugin.node.run(lvl, cam, lwin, lw, lh, buffers=b).copy()
    g_low, g_full = _gpu_guides(plugin, cam, win, pair)
    plugin.set_denoise(sigma_normal=sn, sigma_depth=sz)
    try:
        for name, low in (("checker", sy.frame("checker", g_low)), ("rendered", rendered)):
            want, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam, sigma_n=sn, sigma_z=sz)
            want64, _ = u64.upscale_frame(oracle, low, g_low, g_full, cam, sigma_n=sn, sigma_z=sz)
            assert (stage == ur.STAGE_A).sum() >= sy.MIN_PIXELS and (stage == ur.STAGE_B).sum() >= sy.MIN_PIXELS      # the weighted stages
            got = _upscale(plugin, cam, win, lw, lh, low, w, h).view(F32)
            err = _check_against(got, want, stage, (sigmas, name), want64)
            print(f"sigma_normal {sn:g} sigma_depth {sz:g} {name}: max err {err:.3g}")
    finally:
        plugin.set_denoise()


def _mask(plugin, cam, win, lw, lh, low, w, h):
    import torch
    d_low = _device(low)
    m = torch.full((h + 1, w), 0x55, dtype=torch.uint8, device="cuda")
    plugin.node.upscale_refine_mask_device(cam, win, lw, lh, d_low.data_ptr(), w, h, m.data_ptr())
    torch.cuda.synchronize()
    got = m.cpu().numpy()
    assert (got[h] == 0x55).all(), "guard row"
    return got[:h]


@functools.lru_cache(maxsize=None)
def _full_frame(oracle, pair):
    """The oracle's full-size frame of the refine view: shared, never written."""
    w, h = pair[:2]
    lvl, cam, win, _ = _view(pair, 4, 4)
    full, _ = oracle.render(_scene(brt.SCENE_COVER), lvl, cam, win, w, h)
    full.setflags(write=False)
    return full


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["checker", "blocks2", "all_nan"])
@pytest.mark.parametrize("pair", REFINE_PAIRS, ids=sy.pair_id)
def test_mask_and_list_forms_on_synthetic_frames(plugin, oracle, pair, pattern):
    """The mask is the restatement's classes (EDGES where stage A has no eligible tap -- which now depends on the finiteness of the
    caller's low frame --, SPECULAR from the material, 0 on the sky); under every class set the re-traced pixels are exactly the masked
    set (the count word, and the oracle's full-size frame on them) and every other pixel is bitwise the plain kernel's."""
    import torch
    w, h, lw, lh = pair
    b = _scene(brt.SCENE_COVER)
    lvl, cam, win, _ = _view(pair, 4, 4)
    plugin.node.write_buffers(b)
    g_low, g_full = _gpu_guides(plugin, cam, win, pair)
    low = sy.frame(pattern, g_low)
    _, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
    sy.check_conditions(pattern, stage, pair)
    want = rr.class_mask(stage, g_full, b.materials)
    hit = stage != ur.SKY
    assert not want[~hit].any() and ((want & rr.SPECULAR) != 0).any()
    if pattern == "all_nan":
        assert ((want[hit] & rr.EDGES) != 0).all()
    got = _mask(plugin, cam, win, lw, lh, low, w, h)
    assert np.array_equal(got, want), (pair, pattern, int((got != want).sum()))
    plain = _upscale(plugin, cam, win, lw, lh, low, w, h)
    full = np.ascontiguousarray(_full_frame(oracle, pair)).view(np.uint8).reshape(h, w, -1)
    for classes in (rr.EDGES, rr.SPECULAR, rr.EDGES | rr.SPECULAR):
        sel = rr.selected(want, classes)
        assert sel.any() and (~sel).any()
        d_low, out = _device(low), _guarded(w, h, brt.FLAG_OUT_RGBA32F)
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        plugin.node.upscale_refine_device(cam, win, lw, lh, d_low.data_ptr(), w, h, out.data_ptr(), classes, count.data_ptr())
        refined = _frame_of(out, w, h)
        assert int(count.cpu()[0]) == int(sel.sum()), (pair, pattern, classes)
        assert _same_bits(refined[sel], full[sel]), (pair, pattern, classes, "re-traced")
        assert _same_bits(refined[~sel], plain[~sel]), (pair, pattern, classes, "the plain kernel's")


@pytest.mark.gpu
def test_blended_form_on_blocks2(plugin, oracle):
    """Level 2 with the raster fixture of tests/test_upscale_blend.py: a covered pixel is its texel, any other pixel is bitwise the
    plain kernel's on the same synthetic frame -- stages B and C and the zero store among them -- in f32 and in srgb8."""
    pair = (96, 54, 48, 27)
    w, h, lw, lh = pair
    b = _scene(brt.SCENE_COVER)
    lvl, cam, win = uniforms(w, h, 2, 2, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0), 0.5, 0.5, level=brt.Raytracing.FallbackRaytraced)
    plugin.node.write_buffers(brt.Buffers(b.models, b.materials, None))
    g_low, g_full = _gpu_guides(plugin, cam, win, pair)
    low = sy.frame("blocks2", g_low)
    _, stage = ur.upscale_frame(oracle, low, g_low, g_full, cam)
    rgba, depth = ubr.raster_rgba(w, h), ubr.raster_depth(w, h)
    cov = ubr.covered(cam, 2, g_full[..., 3], depth)
    counts = sy.stage_counts(stage[~cov])
    print(f"blocks2 96x54 from 48x27, level 2: covered {ubr.class_shares(cov)[0]:.4f}, uncovered sky / A / B / C / none {counts}")
    assert min(ubr.class_shares(cov)) >= 0.20
    assert counts[ur.STAGE_A] >= sy.MIN_PIXELS and counts[ur.STAGE_B] >= sy.MIN_PIXELS and counts[ur.STAGE_C] >= sy.MIN_PIXELS and counts[ur.STAGE_NONE] >= 1
    d_low, d_rgba, d_depth = _device(low), _device(rgba), _device(depth)
    for fmt, name in FORMATS[:2]:
        plain = _upscale(plugin, cam, win, lw, lh, low, w, h, fmt)
        out = _guarded(w, h, fmt)
        plugin.node.upscale_blend_device(lvl, cam, win, lw, lh, d_low.data_ptr(), w, h, out.data_ptr(), d_raster_rgba=d_rgba.data_ptr(),
                                         d_raster_depth=d_depth.data_ptr(), out_format=fmt)
        got = _frame_of(out, w, h)
        tex = np.ascontiguousarray(rgba if name is None else oracle.encode_frame(rgba, name)).view(np.uint8).reshape(h, w, -1)
        assert np.array_equal(got[cov], tex[cov]), name
        assert np.array_equal(got[~cov], plain[~cov]), name
